// errors.h -- how every file of the library reports an error: the code is returned, the text goes to the calling
// thread's gcwt_last_error() string, which api.cpp owns.
#pragma once
#include <exception>
#include <new>
#include <string>

#include "../../include/ghostcwt.h"

int gcwt_internal_set_error(int code, const char* msg);   // api.cpp (C++ linkage)

namespace gcwt {

inline int fail(int code, const std::string& msg) { return gcwt_internal_set_error(code, msg.c_str()); }

// Nothing may unwind across the C ABI: entry points that allocate run inside this.
template <typename F>
int guarded(F&& body) {
  try {
    return body();
  } catch (const std::bad_alloc&) {
    return fail(GCWT_ERR_NOMEM, "out of host memory");
  } catch (const std::exception& e) {
    return fail(GCWT_ERR_INVALID, std::string("internal error: ") + e.what());
  } catch (...) {
    return fail(GCWT_ERR_INVALID, "internal error");
  }
}

}  // namespace gcwt
