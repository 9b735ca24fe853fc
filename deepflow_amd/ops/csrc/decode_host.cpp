// Host build of the ingest decoders: the same decode_l7_record /
// decode_l4_record that k_decode_l7 / k_decode_l4 run per thread, looped
// over the records on host pointers. Part of libdfcpu.so; exists so the
// parsers can be tested (and fuzzed under a sanitizer) without a GPU.
//
// Arguments are those of df_decode_l7 / df_decode_l4 minus the stream.
// `payload` must be 8-byte aligned and its allocation must reach the next
// 8-byte boundary (ByteStream, pb_stream.h).
#define DF_HOST_BUILD 1
#include "l7_decode.h"
#include "l4_decode.h"

extern "C" {

int df_decode_l7_host(const void* payload, const void* offs, const void* lens,
                      uint32_t n,
                      void* u64c, void* u32c, void* u8c, void* strc,
                      void* attrc, void* attr_cnt,
                      uint64_t stride, uint64_t base_row,
                      uint64_t scratch_stride) {
    L7Cols cols{(uint64_t*)u64c, (uint32_t*)u32c, (uint8_t*)u8c, (uint64_t*)strc,
                (uint64_t*)attrc, (uint8_t*)attr_cnt, stride, base_row,
                scratch_stride};
    ByteStream bs;
    bs.init((const uint8_t*)payload);
    for (uint32_t rid = 0; rid < n; rid++)
        decode_l7_record(bs, ((const uint32_t*)offs)[rid],
                         ((const uint32_t*)lens)[rid], rid, cols);
    return 0;
}

int df_decode_l4_host(const void* payload, const void* offs, const void* lens,
                      uint32_t n, void* u64c, void* u32c, void* u8c, void* strc,
                      uint64_t stride, uint64_t base_row,
                      uint64_t scratch_stride) {
    L4Cols cols{(uint64_t*)u64c, (uint32_t*)u32c, (uint8_t*)u8c,
                (uint64_t*)strc, stride, base_row, scratch_stride};
    ByteStream bs;
    bs.init((const uint8_t*)payload);
    for (uint32_t rid = 0; rid < n; rid++)
        decode_l4_record(bs, ((const uint32_t*)offs)[rid],
                         ((const uint32_t*)lens)[rid], rid, cols);
    return 0;
}

}  // extern "C"
