/* TEST INFRASTRUCTURE ONLY: the two emulator drivers the stand-in library links, as ONE translation unit (both include
   csrc/gz_emit.h, whose kernels are ordinary functions on the emulator: two objects would define them twice). */
#include "../emu_bamgz/driver.cpp"
#include "../emu_bgzf/driver.cpp"
