/*
 * bamout_stand_in.cpp -- TEST INFRASTRUCTURE ONLY (tests/stub_bamout/libfastplong_amd.so, built by tests/stub_bamout/build.py).
 *
 * The CPU stand-in of tests/stub (fpl_stub.cpp, unchanged: compiled into this translation unit so that its queue can be seen)
 * plus the gzip entry points of ABI v9, fpl_set_gzip_framing AND fpl_set_gzip_records (../stub/gzip_stand_in.h): one gzip member
 * per batch, or, with FPL_GZIP_BGZF or FPL_GZIP_BAM, BGZF blocks of 49 152 bytes each, of FASTQ text or of BAM records.
 */
#define STAND_IN_FRAMING
#define STAND_IN_RECORDS
#include "../stub/fpl_stub.cpp"
#include "../stub/gzip_stand_in.h"
