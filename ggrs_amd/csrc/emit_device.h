// emit_device.h -- device routines shared by the two send sides of the P2P engine's wire protocol,
// p2p_emit.hip (a session's endpoint towards its peers) and p2p_spec_emit.hip (its endpoints towards
// its spectators): the streaming bitfield-rle writer, the bincode framing of an encoded packet row,
// the coalesced write-out of a group of packet rows from LDS, and the fill of the per-session words
// before the first call.  The host side both units share is p2p_engine.h's PacketEmitState.  (An
// endpoint's pop, send decision and encode loop stay written in each kernel: through shared inline
// functions packet emit measured 2-3 % slower per call in every form tried)
// Wire format: see codec.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "codec_device.h"
#include "common.h"
#include "p2p_engine.h"

namespace ggrs {
namespace {

static_assert(kEmitBlock == 64, "the write-out loop splits a group row index by 6 bits");
constexpr int kEmitHeader = 9;  // input_sizes' tag and encoded_bytes' length before the runs

// bitfield-rle over a byte stream fed one byte at a time, into an LDS row (bounded by `room`:
// ggrs_codec_max_packet_bytes covers every stream, the bound only keeps a wrong length in the row).
// A literal stretch is written one byte past its start; its header is one byte for up to 63
// bytes, else the stretch moves up a byte when it ends.
struct RunWriter {
  uint8_t* out;
  int32_t room;
  int32_t pos = 0;
  int32_t run = 0;    // bytes in the open run
  int32_t kind = -1;  // -1 none, 0 zeros, 1 0xFF, 2 literal
  __device__ inline void put(int32_t at, uint8_t v) {
    if (at < room) out[at] = v;
  }
  __device__ inline void varint(uint32_t v) {
    do {
      const uint8_t b = v & 0x7f;
      v >>= 7;
      put(pos++, b | (v ? 0x80 : 0));
    } while (v);
  }
  __device__ inline void close() {
    if (kind < 0) return;
    if (kind < 2) {
      varint(((uint32_t)run << 2) | (kind == 1 ? 2u : 0u) | 1u);
    } else {
      const uint32_t h = (uint32_t)run << 1;
      if (h < 0x80u) {
        put(pos, (uint8_t)h);
        pos += 1 + run;
      } else {  // (run <= 384: two header bytes)
        for (int32_t i = run; i >= 1; --i)
          if (pos + i < room) put(pos + 1 + i, out[pos + i]);
        put(pos, (uint8_t)(h & 0x7f) | 0x80);
        put(pos + 1, (uint8_t)(h >> 7));
        pos += 2 + run;
      }
    }
    kind = -1;
    run = 0;
  }
  __device__ inline void byte(uint8_t x) {
    const int32_t k = x == 0x00 ? 0 : (x == 0xFF ? 1 : 2);
    if (k != kind) {
      close();
      kind = k;
    }
    if (k == 2) put(pos + 1 + run, x);
    ++run;
  }
};

// The bincode framing in front of a row's runs (`rle_bytes` of them, written from row + kEmitHeader);
// returns the packet's length, bounded by the row
__device__ inline int32_t emit_frame_row(uint8_t* row, int32_t rle_bytes, int32_t stride) {
  row[0] = 0;  // input_sizes: None (every input is the reference's size, compression.rs:27-35)
#pragma unroll
  for (int b = 0; b < 4; b++) {  // encoded_bytes' length, a u64
    row[1 + b] = (uint8_t)((uint32_t)rle_bytes >> (8 * b));
    row[5 + b] = 0;
  }
  return min(kEmitHeader + rle_bytes, stride);
}

// A group's rows out, coalesced: LDS rows [gn][kEmitBlock] at `pitch` bytes with their packet lengths
// l_len[gn * kEmitBlock] go to the output rows (first_row + g) * S + s0 + r of `stride` bytes.  Dword
// q is column q & (2^sh - 1) of row q >> sh -- the longest packet's dwords (maxdw <= stride / 4)
// rounded up to a power of two, so that no index needs a division; a row's dwords past its own packet
// are not written, nor the rows of the block's sessions past S (r >= nb).
__device__ inline void emit_write_group(const uint8_t* rows, const int32_t* l_len, int pitch, int gn, int nb, int maxdw,
                                        uint8_t* o_packets, int64_t first_row, int64_t S, int64_t s0, int32_t stride,
                                        int t) {
  if (!maxdw) return;
  const int sh = maxdw > 1 ? 32 - __clz(maxdw - 1) : 0;
  const int total = (gn * kEmitBlock) << sh;
#pragma unroll 4
  for (int q = t; q < total; q += kEmitBlock) {
    const int rowi = q >> sh, cc = q & ((1 << sh) - 1);
    const int gg = rowi >> 6, r = rowi & (kEmitBlock - 1);
    if (r < nb && cc < ((l_len[rowi] + 3) >> 2)) {
      uint32_t* dst = reinterpret_cast<uint32_t*>(o_packets + ((first_row + gg) * S + s0 + r) * stride);
      dst[cc] = reinterpret_cast<const uint32_t*>(rows + (size_t)rowi * pitch)[cc];
    }
  }
}

// The emits' per-session words before the first call: the fields in zero_mask 0, the rest NULL_FRAME
// ([fields][rows])
__global__ void emit_fill_kernel(int32_t* st, int64_t rows, int fields, uint32_t zero_mask) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < (int64_t)fields * rows) st[i] = (zero_mask >> (int)(i / rows)) & 1u ? 0 : GGRS_NULL_FRAME;
}
inline int emit_fill(int32_t* st, size_t rows, int fields, uint32_t zero_mask, hipStream_t stream) {
  emit_fill_kernel<<<grid_of((int64_t)fields * (int64_t)rows, 256), 256, 0, stream>>>(st, (int64_t)rows, fields, zero_mask);
  HIP_TRY(hipGetLastError());
  return GGRS_OK;
}

}  // namespace
}  // namespace ggrs
