// synctest_sincos_block.h -- the rotations of one 8-step core block of the check_distance-8,
// two-player SyncTest kernel (engine.hip, synctest_pipelined_v5_kernel<2, true>) and their sin/cos,
// evaluated once per block by the producer wave instead of once per step.  Also run, as it
// stands, by tests/native/sincos_block_kat_device.hip.
//
// A wave holds four sessions of 8 chain roles x 2 player lanes: lane = session * 16 + role * 2 +
// player (synctest_save.h).  In a core step every role of a session holds the same state, and a
// step's new rot depends on nothing but the old rot and the step's InputRec:
//     a = rot + delta;  rot = a + (a < 0 ? 2pi : a >= thr ? -2pi : 0)         (advance_player_rec_q)
// All eight records of a block are in registers at its head, so every lane can run the eight turns
// of the block at once (block_rot_chain): r[u] is the rot after step u's turn, the rot step u + 1
// starts from.  The sin/cos a step needs is that of the rot it starts from, so the eight values a
// block's steps 1..7 and the next block's step 0 need are the sin/cos of r[0..7]: the lane of role
// j evaluates glibc_sincosf_domain_raw(r[j]) -- one polynomial pass per block on every lane
// instead of eight -- and publishes it as one 16-byte entry (sr, cr, qs, qc) in LDS; step u + 1
// reads the entry of lane (its session, role u, its player).
//
// Why the results are what one evaluation per step gave:
//   * the turns are the two f32 operations of advance_player_rec_q, in its order, with its compare
//     forms, on the same operands (the lane's own rot at the block's head, then its own r[u - 1]):
//     r[u] is bit for bit the rot the per-step form held after step u.  The per-step form rotated
//     rot one role up after every step; with all roles equal that move changes no value.
//   * glibc_sincosf_domain_raw is called unchanged, on r[j]; the per-step form called it on the
//     same value (the hook saw r[u] before the role rotation, every role's r[u] being equal), so
//     the entry's four words are the four values step u + 1 held in registers.
//   * nothing else in the step reads rot (advance_player_rec_q_turned is the same text without the
//     turn), and field 4 of the hand-off is r[u], as before.
//   * roles that differ (which the per-step form's rotation would have carried from role to role):
//     every lane still hands over its own rot of every step, so synctest_save_block's comparison
//     raises the launch's flag exactly when some role's field differs at some step, and the host
//     replays the launch on the sequential kernel; nothing the flagged launch stored survives.
//     A lane then may have read an entry computed from another role's differing rot: only in a
//     launch that is discarded.
//
// The kernel's pass goes one step further (increment_block_pass).  All a step does with the four
// words is fold them with (sgn, keep) of its own record into the velocity increment (ix, iy)
// (box_game.h, rec_q_increment) -- eight times per lane and block, though it depends on nothing a
// lane owns.  The lane of role j holds the record of the step that reads its entry: its batch
// sub-step's, row t + j + 1, in a register at the block's head.  So it computes the increment once
// and publishes those 8 bytes; a core step reads them and adds them, and no record reaches it.
//
// Why the results are what the increment computed inside every step gave:
//   * (ix, iy) is a pure function of the entry's four words and (sgn, keep) of row t + u + 1;
//     rec_q_increment is the text the per-step form ran (advance_player_rec_q is now that function
//     followed by advance_player_inc_body), the same operations on the same operands in the same
//     order -- including the increment (-0.0, -0.0) when keep is 0;
//   * row t + u + 1 is the row step u + 1 read its record from: the lane of role u reads it with
//     the same index expression as its batch record, and role 7's is row t + 8, the next block's
//     step 0 (carried in two registers; before the first block, the evaluation in front of the
//     loop folded with that block's step-0 record);
//   * the consumer's batch sub-step of role j starts from the hand-off of step j and takes row
//     t + j + 1: its increment is the lane's own entry, its turn the record's (delta, thr);
//   * roles that differ still hand over their own fields at every step, synctest_save_block raises
//     the flag, and the launch is replayed on the sequential kernel, as above.
// sincos_block_pass and sincos_block_entry, the 16-byte form, stay as the KAT of the pass's shared
// part (tests/native/sincos_block_kat_device.hip); the kernel runs the increment form
// (tests/native/increment_block_kat_device.hip).
//
// The select of r[j] by role costs no compare/select ladder: the eight r[u] go where the hand-off's
// field-4 words of the block's eight slots go anyway, and the lane reads its own word of slot j back
// (the same lane, the same address class: the wave's LDS queue is in order).
#pragma once
#include <hip/hip_runtime.h>

#include "box_game.h"
#include "glibc_sincosf.h"
#include "synctest_save.h"

namespace ggrs {

constexpr int kSincosEntry = 16;                       // (sr, cr, qs, qc)
constexpr int kSincosBlockBytes = kWave * kSincosEntry;  // one block's entries, one per lane
constexpr int kIncEntry = 8;                            // (ix, iy): the kernel's entries
constexpr int kIncBlockBytes = kWave * kIncEntry;

// r[u]: the rot after step u's turn, from the rot at the block's head and (delta, thr) of the
// block's records, which is all a turn reads of a record.
__device__ __forceinline__ void block_rot_chain(float rot0, const uint2 (&turn)[kSaveCd], float (&r)[kSaveCd]) {
  float rot = rot0;
#pragma unroll
  for (int u = 0; u < kSaveCd; u++) {
    const float a = rot + __builtin_bit_cast(float, turn[u].x);
    rot = a + (a < 0.0f ? kTwoPi : (a >= __builtin_bit_cast(float, turn[u].y) ? -kTwoPi : 0.0f));
    r[u] = rot;
  }
}
// The same from whole records.
__device__ __forceinline__ void block_rot_chain(float rot0, const InputRec (&rec)[kSaveCd], float (&r)[kSaveCd]) {
  uint2 turn[kSaveCd];
#pragma unroll
  for (int u = 0; u < kSaveCd; u++) turn[u] = make_uint2(rec[u].delta, rec[u].thr);
  block_rot_chain(rot0, turn, r);
}

// The part every form of the pass shares: the field-4 words of the block's eight slots, the lane's
// own r[j] read back, and its sin/cos.  hb: the block's hand-off buffer (kSaveHandBytes); wl, j: the
// lane and its role.
__device__ __forceinline__ void block_rot_eval(uint8_t* hb, int wl, int j, const float (&r)[kSaveCd], float* s, float* c,
                                               uint32_t* qs, uint32_t* qc) {
  uint8_t* own = hb + kWave * 16 + wl * 4;  // the lane's field-4 word of slot 0
#pragma unroll
  for (int u = 0; u < kSaveCd; u++) *reinterpret_cast<uint32_t*>(own + u * kSaveHandSlot) = __builtin_bit_cast(uint32_t, r[u]);
  const uint32_t rj = *reinterpret_cast<const uint32_t*>(own + j * kSaveHandSlot);
  glibc_sincosf_domain_raw(__builtin_bit_cast(float, rj), s, c, qs, qc);
}
// The entry lane (session, role u, player) wrote, seen from lane wl of role j.
template <typename T>
__device__ __forceinline__ T block_entry_of_role(const uint8_t* sc, int wl, int j, int u) {
  return *reinterpret_cast<const T*>(sc + (wl + (u - j) * kSavePlayers) * (int)sizeof(T));
}

// The block's pass with 16-byte entries.  sc: the block's entry buffer (kSincosBlockBytes).  The
// caller orders the entry writes before other lanes' reads (one wave: a compiler fence and the
// wave's in-order LDS queue).
__device__ __forceinline__ void sincos_block_pass(uint8_t* hb, uint8_t* sc, int wl, int j, const float (&r)[kSaveCd]) {
  float s, c;
  uint32_t qs, qc;
  block_rot_eval(hb, wl, j, r, &s, &c, &qs, &qc);
  *reinterpret_cast<uint4*>(sc + wl * kSincosEntry) = make_uint4(__builtin_bit_cast(uint32_t, s), __builtin_bit_cast(uint32_t, c), qs, qc);
}

// What step u + 1 of the block (u = 7: step 0 of the next block) needs on lane wl of role j: the
// entry of lane (session, role u, player), one 16-byte read.
__device__ __forceinline__ uint4 sincos_block_entry(const uint8_t* sc, int wl, int j, int u) {
  return block_entry_of_role<uint4>(sc, wl, j, u);
}

// The pass the kernel runs: the lane of role j also holds the record of the step that reads its
// entry (row t + j + 1, the record its batch sub-step takes), so it finishes the job and publishes
// that step's velocity increment, 8 bytes (ix, iy), instead of the sin/cos.  sgn, keep: that
// record's.  sc: kIncBlockBytes.
__device__ __forceinline__ void increment_block_pass(uint8_t* hb, uint8_t* sc, int wl, int j, const float (&r)[kSaveCd],
                                                     uint32_t sgn, uint32_t keep) {
  float s, c;
  uint32_t qs, qc;
  block_rot_eval(hb, wl, j, r, &s, &c, &qs, &qc);
  const VelInc inc = rec_q_increment(s, c, qs, qc, sgn, keep);
  *reinterpret_cast<uint2*>(sc + wl * kIncEntry) = make_uint2(inc.ix, inc.iy);
}

// The increment of step u + 1 of the block (u = 7: of step 0 of the next block) on lane wl of role
// j: the entry of lane (session, role u, player), one 8-byte read.
__device__ __forceinline__ VelInc increment_block_entry(const uint8_t* sc, int wl, int j, int u) {
  const uint2 e = block_entry_of_role<uint2>(sc, wl, j, u);
  return VelInc{e.x, e.y};
}

}  // namespace ggrs
