/* oracle/standin/isa-l/igzip_lib.h -- TEST INFRASTRUCTURE ONLY.
 *
 * Declarations of the ISA-L inflate interface, as far as the reference's FASTQ reader uses it, so that the reference
 * compiles without the library.  The functions are defined in oracle/standin/isal_stub.cpp, which refuses gzip input:
 * the reference build made from these files reads plain-text FASTQ only. */
#ifndef FPL_STANDIN_IGZIP_LIB_H
#define FPL_STANDIN_IGZIP_LIB_H
#include <stddef.h>
#include <stdint.h>

#define ISAL_DECOMP_OK 0
#define ISAL_BLOCK_FINISH 4
#define ISAL_GZIP_NO_HDR_VER 3

struct isal_gzip_header {
    uint32_t text, time, xflags, os;
    uint8_t* extra;
    uint32_t extra_buf_len, extra_len;
    char* name;
    uint32_t name_buf_len;
    char* comment;
    uint32_t comment_buf_len;
    uint32_t hcrc, flags;
};

struct inflate_state {
    uint8_t* next_out;
    uint32_t avail_out;
    uint32_t total_out;
    uint8_t* next_in;
    uint32_t avail_in;
    uint64_t read_in;
    int32_t read_in_length;
    uint32_t block_state;
    uint32_t bfinal;
    uint32_t crc_flag;
    uint32_t crc;
};

#ifdef __cplusplus
extern "C" {
#endif
void isal_inflate_init(struct inflate_state* state);
void isal_inflate_reset(struct inflate_state* state);
void isal_gzip_header_init(struct isal_gzip_header* header);
int isal_read_gzip_header(struct inflate_state* state, struct isal_gzip_header* header);
int isal_inflate(struct inflate_state* state);
#ifdef __cplusplus
}
#endif
#endif
