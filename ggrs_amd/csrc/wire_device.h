// wire_device.h -- device routines shared by the two kernels of the wire envelope (wire.hip): the
// staging of a block's rows between global memory and LDS with coalesced dword accesses, moving only
// as many dwords per row as the block's longest row needs, and the reads and writes of little-endian
// fields at unaligned offsets of an LDS row.  Wire format: see wire.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "codec_device.h"
#include "common.h"

namespace ggrs {
namespace {

constexpr int kWireBlock = 64;              // threads per block: one wave
constexpr size_t kWireLds = 64 * 1024;      // a block's datagram rows and packet rows must fit
constexpr int32_t kWireMaxDgram = 2048;     // the longest datagram row
constexpr int32_t kWireMaxPacket = 1012;    // the longest packet row (the packet feeds' bound)
constexpr int32_t kWireHeader = 6;          // magic u16, tag u32
constexpr int32_t kWireInputFixed = 31;     // an Input message without its statuses and bytes

// LDS rows keep one dword past the row, so that a dword assembled from two neighbours never reads
// outside its row, at an odd dword pitch (codec_device.h)
__host__ __device__ constexpr int wire_pitch(int bytes) { return odd_dword_pitch(bytes + 4); }

// The sessions a block takes: the largest power of two, at most one per thread, whose rows fit
inline int wire_sessions_per_block(int32_t dgram_stride, int32_t packet_stride) {
  const size_t per = (size_t)wire_pitch(dgram_stride) + (size_t)wire_pitch(packet_stride) + sizeof(int32_t);
  int nb = kWireBlock;
  while (nb > 1 && (size_t)nb * per > kWireLds) nb >>= 1;
  return nb;
}
inline size_t wire_lds_bytes(int nb, int32_t dgram_stride, int32_t packet_stride) {
  return (size_t)nb * ((size_t)wire_pitch(dgram_stride) + (size_t)wire_pitch(packet_stride) + sizeof(int32_t));
}

// bytes [shift, shift + 4) of the eight bytes lo, hi
__device__ inline uint32_t wire_align(uint32_t hi, uint32_t lo, uint32_t shift) {
  return __builtin_amdgcn_alignbyte(hi, lo, shift);
}
// Little-endian fields at any offset of a dword-aligned LDS row (off + 4 <= the row's bytes, so the
// second dword is at most the row's spare one)
__device__ inline uint32_t wire_ld32(const uint8_t* row, int off) {
  const uint32_t* w = reinterpret_cast<const uint32_t*>(row) + (off >> 2);
  return wire_align(w[1], w[0], (uint32_t)off & 3u);
}
__device__ inline uint64_t wire_ld64(const uint8_t* row, int off) {
  return (uint64_t)wire_ld32(row, off) | (uint64_t)wire_ld32(row, off + 4) << 32;
}
__device__ inline void wire_st32(uint8_t* row, int off, uint32_t v) {
#pragma unroll
  for (int b = 0; b < 4; b++) row[off + b] = (uint8_t)(v >> (8 * b));
}

// The block's maximum of v (>= 0); the barriers also order the block's LDS rows around it
__device__ inline int wire_block_max(int v, int* s_max) {
  __syncthreads();
  if (threadIdx.x == 0) *s_max = 0;
  __syncthreads();
  if (v > 0) atomicMax(s_max, v);
  __syncthreads();
  return *s_max;
}

// `rows` rows of row_bytes bytes, contiguous from src (dword aligned), -> LDS rows at `pitch` bytes:
// the first maxdw (<= row_bytes / 4) dwords of each.  Dword q is column q & (2^sh - 1) of row q >> sh,
// the row length rounded up to a power of two, so that no index needs a division.
__device__ inline void wire_rows_in(uint8_t* lds, int pitch, const uint8_t* src, int32_t row_bytes, int rows, int maxdw) {
  if (!maxdw) return;
  const int sh = maxdw > 1 ? 32 - __clz(maxdw - 1) : 0;
  const int sdw = row_bytes >> 2, total = rows << sh;
  const uint32_t* s32 = reinterpret_cast<const uint32_t*>(src);
#pragma unroll 4
  for (int q = threadIdx.x; q < total; q += kWireBlock) {
    const int r = q >> sh, cc = q & ((1 << sh) - 1);
    if (cc < maxdw) reinterpret_cast<uint32_t*>(lds + (size_t)r * pitch)[cc] = s32[(int64_t)r * sdw + cc];
  }
}
// ... and back: of row r the dwords that hold its l_len[r] bytes (<= 4 maxdw), no more
__device__ inline void wire_rows_out(uint8_t* dst, int32_t row_bytes, const uint8_t* lds, int pitch, const int32_t* l_len,
                                     int rows, int maxdw) {
  if (!maxdw) return;
  const int sh = maxdw > 1 ? 32 - __clz(maxdw - 1) : 0;
  const int sdw = row_bytes >> 2, total = rows << sh;
  uint32_t* d32 = reinterpret_cast<uint32_t*>(dst);
#pragma unroll 4
  for (int q = threadIdx.x; q < total; q += kWireBlock) {
    const int r = q >> sh, cc = q & ((1 << sh) - 1);
    if (cc < ((l_len[r] + 3) >> 2)) d32[(int64_t)r * sdw + cc] = reinterpret_cast<const uint32_t*>(lds + (size_t)r * pitch)[cc];
  }
}

}  // namespace
}  // namespace ggrs
