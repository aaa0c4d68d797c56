// codec_device.h -- device routines of GGRS's input wire codec (src/network/compression.rs) shared
// by the batch codec (codec.hip), the two packet feeds (through ingest_device.h: p2p_ingest.hip and
// spectator_ingest.hip) and the two send sides (through emit_device.h: p2p_emit.hip and
// p2p_spec_emit.hip): the LEB128 reader, the packet validation (every check of compression::decode,
// in the reference's order), the run expansion of an already validated packet and the LDS row pitch.
// Wire format: see codec.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.h"

namespace ggrs {
namespace {

constexpr int64_t kMaxDecoded = 1 << 24;  // oracle/codec.c CODEC_MAX_DECODED

__device__ inline bool get_varint(const uint8_t* in, int64_t n, int64_t& pos, uint64_t& v) {
  uint64_t r = 0;
  for (int shift = 0; shift < 64; shift += 7) {
    if (pos >= n) return false;
    const uint8_t b = in[pos++];
    r |= (uint64_t)(b & 0x7f) << shift;
    if (!(b & 0x80)) {
      v = r;
      return true;
    }
  }
  return false;
}

// LDS rows are padded to an odd number of dwords so that threads stepping through their own rows in
// lockstep spread over the banks.
__host__ __device__ constexpr int odd_dword_pitch(int bytes) {
  int dw = (bytes + 3) / 4;
  if ((dw & 1) == 0) dw += 1;
  return dw * 4;
}

// bincode + bitfield-rle validation of one packet (compression.rs:83-154), the checks of
// decode_kernel in the same order.  On GGRS_CODEC_OK: *cnt inputs, the RLE stream at d + *rle_at
// with *m bytes.
__device__ inline int32_t validate_packet(const uint8_t* d, int64_t len, int stride, int B, int W, int64_t* cnt_out,
                                          uint64_t* m_out, int64_t* rle_at) {
  if (len < 0 || len > stride) return GGRS_CODEC_E_INVALID;
  int64_t pos = 0;
  if (len < 1 || d[0] > 1) return GGRS_CODEC_E_BINCODE;
  const uint8_t tag = d[pos++];
  uint64_t n_sizes = 0;
  int64_t sizes_at = 0;
  if (tag == 1) {
    if (len - pos < 8) return GGRS_CODEC_E_BINCODE;
    for (int b = 0; b < 8; b++) n_sizes |= (uint64_t)d[pos + b] << (8 * b);
    pos += 8;
    if (n_sizes > (uint64_t)(len - pos) / 4) return GGRS_CODEC_E_BINCODE;
    sizes_at = pos;
    pos += 4 * (int64_t)n_sizes;
  }
  if (len - pos < 8) return GGRS_CODEC_E_BINCODE;
  uint64_t m = 0;
  for (int b = 0; b < 8; b++) m |= (uint64_t)d[pos + b] << (8 * b);
  pos += 8;
  if (m > (uint64_t)(len - pos)) return GGRS_CODEC_E_BINCODE;
  const uint8_t* rle = d + pos;
  int64_t xl = 0;
  for (int64_t q = 0; q < (int64_t)m;) {
    uint64_t h;
    if (!get_varint(rle, (int64_t)m, q, h)) return GGRS_CODEC_E_RLE;
    const uint64_t rl = (h & 1) ? h >> 2 : h >> 1;
    if (rl > (uint64_t)kMaxDecoded || (uint64_t)xl + rl > (uint64_t)kMaxDecoded) return GGRS_CODEC_E_RLE;
    if (!(h & 1)) {
      if ((uint64_t)((int64_t)m - q) < rl) return GGRS_CODEC_E_RLE;
      q += (int64_t)rl;
    }
    xl += (int64_t)rl;
  }
  int64_t cnt;
  bool all_b = true;
  if (tag == 1) {
    cnt = (int64_t)n_sizes;
    int64_t bs = B, sum = 0;
    for (int64_t k = 0; k < cnt; k++) {
      uint32_t u = 0;
      for (int b = 0; b < 4; b++) u |= (uint32_t)d[sizes_at + 4 * k + b] << (8 * b);
      const int64_t sz = (int64_t)(int32_t)((uint32_t)bs + u);
      if (sz < 0) return GGRS_CODEC_E_DELTA;
      all_b &= sz == B;
      bs = sz;
      sum += sz;
      if (sum > xl) return GGRS_CODEC_E_DELTA;
    }
    if (sum != xl) return GGRS_CODEC_E_DELTA;
  } else {
    cnt = xl / B;
    if (cnt * B != xl) return GGRS_CODEC_E_DELTA;
  }
  if (!all_b) return GGRS_CODEC_UNSUPPORTED;
  if (cnt > W) return GGRS_CODEC_E_CAP;
  *cnt_out = cnt;
  *m_out = m;
  *rle_at = pos;
  return GGRS_CODEC_OK;
}

// The run expansion of a packet validate_packet accepted (bitfield_rle::decode's second pass,
// compression.rs:91): every byte of the XOR-delta stream, in order, to `sink` -- the codec kernels'
// loop (decode_kernel) with the store left to the caller, so a consumer that keeps the previous
// input in registers needs no dense buffer.  The stream is at most W * B bytes (validate_packet).
template <typename Sink>
__device__ inline void expand_runs(const uint8_t* rle, int64_t m, Sink&& sink) {
  int64_t q = 0;
  while (q < m) {
    uint64_t h;
    if (!get_varint(rle, m, q, h)) return;  // (validated: never taken)
    const int64_t rl = (int64_t)((h & 1) ? h >> 2 : h >> 1);
    if (h & 1) {
      const uint8_t fill = (h & 2) ? 0xFF : 0x00;
      for (int64_t k = 0; k < rl; k++) sink(fill);
    } else {
      if (m - q < rl) return;  // (validated: never taken)
      for (int64_t k = 0; k < rl; k++) sink(rle[q + k]);
      q += rl;
    }
  }
}

}  // namespace
}  // namespace ggrs
