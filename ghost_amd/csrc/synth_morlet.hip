// synth_morlet.hip -- the complex-gain (Morlet) instantiations of k_synth7, compiled into a code object of their
// own: synth.hip then holds exactly the kernels it holds without them, laid out as they always were (the Morse
// path's instructions and their placement do not change).
#define GCWT_SYNTH_MORLET_TU 1
#include "synth.hip"
