// imm3_order_key.h -- the ONE rule that turns a row's order-key columns into its normalised key: int32 as
// x ^ 0x80000000 big-endian, int8 as x ^ 0x80, strings as they are, a descending key's bytes complemented, zero-padded to 16 bytes;
// unsigned byte order of the key == the order asked for.  Shared by the order itself (imm3_order.hip) and by the merge of ordered
// results (imm3_merge_order.hip), which builds the same key again from the ORDERED columns.
#ifndef IMM3_ORDER_KEY_H
#define IMM3_ORDER_KEY_H
#include "imm3_internal.h"

#include <hip/hip_runtime.h>

namespace imm3 {

// the normalised key of row i of the columns `cols[c].src`: key byte 0 in the top byte of k[0]
__device__ inline void order_build_key(const OrderKeyCol *cols, int n_cols, int key_bytes, int64_t i, uint32_t k[kOrderKeyWords]) {
    unsigned long long hi = 0, lo = 0;
    auto push = [&](uint32_t byte) {
        hi = (hi << 8) | (lo >> 56);
        lo = (lo << 8) | (unsigned long long)(byte & 0xFFu);
    };
    for (int c = 0; c < n_cols; ++c) {
        const OrderKeyCol &col = cols[c];
        const uint32_t flip = col.descending ? 0xFFu : 0u;
        if (col.kind == KIND_I32) {
            const uint32_t v = ((const uint32_t *)col.src)[i] ^ 0x80000000u;
            push((v >> 24) ^ flip);
            push((v >> 16) ^ flip);
            push((v >> 8) ^ flip);
            push(v ^ flip);
        } else if (col.kind == KIND_I8) {
            push(((uint32_t)col.src[i] ^ 0x80u) ^ flip);
        } else {
            const uint8_t *p = col.src + i * col.width;
            for (int b = 0; b < col.width; ++b) push((uint32_t)p[b] ^ flip);
        }
    }
    for (int b = key_bytes; b < kOrderKeyMaxBytes; ++b) push(0u);
    k[0] = (uint32_t)(hi >> 32);
    k[1] = (uint32_t)hi;
    k[2] = (uint32_t)(lo >> 32);
    k[3] = (uint32_t)lo;
}

} // namespace imm3
#endif
