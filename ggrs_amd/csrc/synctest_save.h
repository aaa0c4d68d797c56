// synctest_save.h -- the saves of one 8-step core block of the check_distance-8, two-player SyncTest
// kernel (engine.hip, synctest_pipelined_v5_kernel<2, true>): what its consumer wave does with one
// hand-off buffer.  Also run, as it stands, by tests/native/save_block_kat_device.hip.
//
// A wave holds four sessions of 8 chain roles x 2 player lanes: lane = session * 16 + role * 2 +
// player, a session is one 16-lane DPP row.  In a core step t every role of a session holds the
// post-advance state of the same frame t - cd + 1 (each role replays that frame from the same saved
// state), the step's save goes to one ring cell whatever the role, and SyncTest's comparison asks
// that every role's checksum equal the first one seen.  So a block does, once:
//   1. role equality by state bits: every lane compares its five fields of every step with its
//      neighbour role's (row_ror:2: role j sees role j - 1 of the same player, role 0 sees role 7)
//      and ORs the differences.  All eight roles are equal iff every neighbour pair is.
//   2. one Fletcher pass: lane (session, role j, player) takes step j -- it reads its own entry of
//      hand-off slot j by address and sums it with frame word t + j - cd + 1.
//   3. one save per step: the same lane stores step j's cell into ring slot (sr + j) mod R -- five
//      field stores, one frame-word store (player-0 lanes) and one 16-bit checksum store in which
//      player-0 lanes write ring_ck and player-1 lanes first_ck of their step's slot.  Seven store
//      instructions per block.
//
// Why the results are what one checksum and one save per role gave:
//   * flag clear: every role's bytes were equal at every step, so the bytes stored and their
//     checksums are the ones every role would have stored, and every role's checksum equals the
//     first seen (a checksum is a function of the bytes).
//   * flag set: the host restores the launch's checkpoint and replays the launch on the sequential
//     kernel (resolve()), exactly as after a checksum mismatch; nothing this launch stored survives.
//   * the flag also fires on states that differ but collide in Fletcher-16.  That only costs the
//     replay, which then reports what the reference would (no mismatch).
//   * ggrs_debug_corrupt_on_load never reaches a core block: a launch that holds the corrupted
//     frame runs general steps only.
//
// Stores.  Slot offsets differ per lane, so the whole offset is the vector offset (scalar offset
// 0): the lane's static offset plus slot * slot bytes.  Two conditions, checked where the kernel is
// picked (v5_sessions_per_block):
//   * the eight slots of a block are distinct: R = max_prediction + 1 >= 10 > 8 (check_distance 8
//     < max_prediction), so (sr + j) mod R is one conditional subtract and no two lanes of a
//     session's player write one address in a store instruction;
//   * a lane that must not store has static offset kSaveOob = 2^30; every buffer span is below it
//     (pipe_buffers_fit), so its sum with a slot offset lies in [2^30, 2^31): past the
//     descriptor's num_records, no wrap.
// Consecutive blocks write the same ring cell from different lanes of the same wave, in program
// order: one wave's stores to one address land in order (the kernel depends on the same property
// between its edge steps and its core steps).
#pragma once
#include <hip/hip_runtime.h>

#include "box_game.h"

namespace ggrs {

constexpr uint32_t kSaveOob = 0x40000000u;
constexpr int kSaveCd = 8;                  // check_distance = roles per session = steps per block
constexpr int kSavePlayers = 2;             // player lanes per role
constexpr int kSaveHandSlot = kWave * 20;   // one step's hand-off: a uint4 per lane (fields 0..3), then field 4 per lane
constexpr int kSaveHandBytes = kSaveCd * kSaveHandSlot;
static_assert(kWave == 4 * kSaveCd * kSavePlayers, "a session is one 16-lane DPP row");

// What a lane needs for its saves, fixed for a launch.
struct SaveLane {
  uint32_t fo[5];      // byte offsets of the lane's five fields in ring slot 0 (kSaveOob: no store)
  uint32_t fo_frame;   // of the frame word (player-0 lanes)
  uint32_t co;         // of the 16-bit checksum: ring_ck (player 0) or first_ck (player 1) of slot 0
  uint32_t wt[5];      // doubled Fletcher weights of the five fields
  uint32_t one2;       // doubled byte weights of sum1
  uint32_t wf1, wf2;   // the frame word's (player-0 lanes, else 0)
  uint32_t c1, c2;     // doubled constants of the length prefixes (player-0 lanes, else 0)
  uint32_t slot_bytes, ck_slot_bytes;  // bytes per ring slot: fields, 16-bit checksums
};

// lane (role, player pl) of session s of L; valid: the session exists and runs.  ck_base,
// first_base: byte offsets of ring_ck and first_ck from the ring's base (the descriptor's).
__device__ __forceinline__ SaveLane make_save_lane(bool valid, int pl, int64_t s, int64_t L, uint32_t ck_base,
                                                   uint32_t first_base) {
  constexpr int P = kSavePlayers;
  constexpr int n_bytes = Fletcher<P>::n;
  const int kq[5] = {fld_x(P, pl), fld_y(P, pl), fld_vx(P, pl), fld_vy(P, pl), fld_rot(P, pl)};
  SaveLane c;
#pragma unroll
  for (int q = 0; q < 5; q++) {
    c.fo[q] = valid ? (uint32_t)((kq[q] * L + s) * 4) : kSaveOob;
    c.wt[q] = valid ? 2u * weights_at(n_bytes, fld_offset(P, kq[q])) : 0u;
  }
  c.fo_frame = (valid && pl == 0) ? (uint32_t)(s * 4) : kSaveOob;
  c.co = !valid ? kSaveOob : (pl == 0 ? ck_base : first_base) + (uint32_t)(s * 2);
  c.one2 = valid ? 0x02020202u : 0u;
  c.wf1 = pl == 0 ? 0x02020202u : 0u;
  c.wf2 = pl == 0 ? 2u * weights_at(n_bytes, 0) : 0u;
  c.c1 = pl == 0 ? 2u * Fletcher<P>::kSum1Const : 0u;
  c.c2 = pl == 0 ? 2u * Fletcher<P>::kSum2Const : 0u;
  c.slot_bytes = (uint32_t)(state_fields(P) * L * 4);
  c.ck_slot_bytes = (uint32_t)(L * 2);
  return c;
}

// One core block's saves.  hb: the block's hand-off buffer in LDS (kSaveHandBytes); wl, j: the
// lane and its role; sr: the ring slot of the block's first step (< R); t: that step (its save is
// frame t - cd + 1); valid_lanes: the lanes of sessions that exist and run.  Returns the valid
// lanes that saw a role differ from its neighbour at any step of the block.
__device__ __forceinline__ uint64_t synctest_save_block(const uint8_t* hb, const SaveLane& c,
                                                        __amdgpu_buffer_rsrc_t rs_ring, int R, uint32_t sr, int32_t t,
                                                        int wl, int j, uint64_t valid_lanes) {
  // the lane's own state of every step, against the neighbour role's
  uint32_t acc = 0;
#pragma unroll
  for (int u = 0; u < kSaveCd; u++) {
    const uint4 a = *reinterpret_cast<const uint4*>(hb + u * kSaveHandSlot + wl * 16);
    const uint32_t e = *reinterpret_cast<const uint32_t*>(hb + u * kSaveHandSlot + kWave * 16 + wl * 4);
    const uint32_t v[5] = {a.x, a.y, a.z, a.w, e};
#pragma unroll
    for (int q = 0; q < 5; q++)
      acc |= v[q] ^ (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v[q], 0x122, 0xF, 0xF, true);
  }
  // step j's state: this lane's own entry of slot j (equal to every other role's unless flagged)
  uint32_t w[5];
  {
    const uint8_t* st = hb + (uint32_t)j * kSaveHandSlot;
    const uint4 a = *reinterpret_cast<const uint4*>(st + wl * 16);
    w[0] = a.x, w[1] = a.y, w[2] = a.z, w[3] = a.w;
    w[4] = *reinterpret_cast<const uint32_t*>(st + kWave * 16 + wl * 4);
  }
  const uint32_t frame = (uint32_t)(t + j - kSaveCd + 1);
  uint32_t d1 = dot4_u8(frame, c.wf1, c.c1), d2 = dot4_u8(frame, c.wf2, c.c2);
#pragma unroll
  for (int q = 0; q < 5; q++) {
    d1 = dot4_u8(w[q], c.one2, d1);
    d2 = dot4_u8(w[q], c.wt[q], d2);
  }
  // the two player lanes' sums, on both
  d1 += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)d1, 0xB1, 0xF, 0xF, true);
  d2 += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)d2, 0xB1, 0xF, 0xF, true);
  const uint32_t ck = fletcher_from_doubled(d1, d2);
  uint32_t slot = sr + (uint32_t)j;  // < R + 8 < 2 R
  slot = slot >= (uint32_t)R ? slot - (uint32_t)R : slot;
  const uint32_t so = slot * c.slot_bytes, cso = slot * c.ck_slot_bytes;
#pragma unroll
  for (int q = 0; q < 5; q++) __builtin_amdgcn_raw_buffer_store_b32(w[q], rs_ring, c.fo[q] + so, 0, 0);
  __builtin_amdgcn_raw_buffer_store_b32(frame, rs_ring, c.fo_frame + so, 0, 0);
  __builtin_amdgcn_raw_buffer_store_b16((uint16_t)ck, rs_ring, c.co + cso, 0, 0);
  // (the compare as the wave-wide intrinsic, one v_cmp: as `acc != 0` the optimiser rewrites the
  // OR of xors above into forty compares and selects)
  return __builtin_amdgcn_uicmp(acc, 0u, 33 /* ICMP_NE */) & valid_lanes;
}

}  // namespace ggrs
