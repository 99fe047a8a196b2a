/*
 * bgzfout_stand_in.cpp -- TEST INFRASTRUCTURE ONLY (tests/stub_bgzfout/libfastplong_amd.so, built by tests/stub_bgzfout/build.py).
 *
 * The CPU stand-in of tests/stub (fpl_stub.cpp, unchanged: compiled into this translation unit so that its queue can be seen)
 * plus the gzip entry points of ABI v9 AND fpl_set_gzip_framing (../stub/gzip_stand_in.h): one gzip member per batch, or, with
 * FPL_GZIP_BGZF, BGZF blocks of 49 152 text bytes each.  On purpose it has no fpl_set_gzip_records.
 */
#define STAND_IN_FRAMING
#include "../stub/fpl_stub.cpp"
#include "../stub/gzip_stand_in.h"
