// oracle/standin/isal_stub.cpp -- TEST INFRASTRUCTURE ONLY: the ISA-L entry points declared in isa-l/igzip_lib.h.  The
// reference build links these instead of the library; the first call (only gzip input makes one) ends the run.
#include <cstdio>
#include <cstdlib>

#include "isa-l/igzip_lib.h"

[[noreturn]] static void no_gzip() {
    std::fputs("gzip input is not supported by this reference build\n", stderr);
    std::exit(2);
}

extern "C" {
void isal_inflate_init(struct inflate_state*) { no_gzip(); }
void isal_inflate_reset(struct inflate_state*) { no_gzip(); }
void isal_gzip_header_init(struct isal_gzip_header*) { no_gzip(); }
int isal_read_gzip_header(struct inflate_state*, struct isal_gzip_header*) { no_gzip(); }
int isal_inflate(struct inflate_state*) { no_gzip(); }
}
