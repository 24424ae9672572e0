// synths_morlet.hip -- the complex-gain (Morlet) instantiations of k_synth7s (output stride), in a code object of
// their own like k_synth7's (synth_morlet.hip).
#define GCWT_SYNTH_MORLET_TU 1
#include "synths.hip"
