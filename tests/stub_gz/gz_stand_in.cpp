/*
 * gz_stand_in.cpp -- TEST INFRASTRUCTURE ONLY (tests/stub_gz/libfastplong_amd.so, built by tests/stub_gz/build.py).
 *
 * The CPU stand-in of tests/stub (fpl_stub.cpp, unchanged: compiled into this translation unit so that its queue can be seen)
 * plus the three gzip entry points of ABI v9 (../stub/gzip_stand_in.h): one gzip member per batch, so bin/fastplong_amd's
 * device-gzip path -- the choice of form, members in order, host members between them -- runs on a box without GPUs.  On purpose
 * it has neither fpl_set_gzip_framing nor fpl_set_gzip_records: it is the library that lacks them.
 */
#include "../stub/fpl_stub.cpp"
#include "../stub/gzip_stand_in.h"
