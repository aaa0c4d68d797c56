// p2p_plan.h -- which kernel a P2P advance launches, and how it splits a run into launches: the one
// statement of the selection rules of p2p.hip (fixed latency) and p2p_sched.hip (scheduled arrivals),
// with the LDS geometry those rules size a launch from.  Plain C++17: integer arithmetic on the
// configuration, no HIP runtime header, so a host compiler builds it too (tests/native/p2p_plan_host.cpp).
// The .hip files fill the parameter structs and launch what a plan names; the kernels read the
// geometry below.
#pragma once
#include <stdint.h>
#include <stdlib.h>

#include <algorithm>

#include "ggrs_amd.h"
#include "host_device.h"

namespace ggrs {

// ---- kernel forms (ggrs_p2p_set_unstaged) --------------------------------------------------------

enum class P2PForm : int32_t {
  kDefault = 0,     // canonical flat, or chains for few sessions
  kUnstaged = 1,    // calls in lockstep, input rows read from global memory
  kLockstep = 2,    // calls in lockstep, input rows staged in LDS
  kFlatHbm = 3,     // flat with HBM rings
  kChains = 4,      // chains
  kFlatQueues = 5,  // flat with LDS rings and the queue bookkeeping
  kCanon = 6,       // canonical flat
};

// value, the name ggrs_amd.p2p.P2PEngine.KERNEL_FORMS gives it, and what the ABI's message calls it
struct P2PFormInfo {
  P2PForm form;
  const char* name;
  const char* what;
};
constexpr P2PFormInfo kP2PForms[] = {
    {P2PForm::kDefault, "default", "default"},
    {P2PForm::kUnstaged, "unstaged", "unstaged"},
    {P2PForm::kLockstep, "lockstep", "lockstep"},
    {P2PForm::kFlatHbm, "flat", "flat HBM rings"},
    {P2PForm::kChains, "chains", "chains"},
    {P2PForm::kFlatQueues, "flat_queues", "flat LDS rings with the queue bookkeeping"},
    {P2PForm::kCanon, "canonical", "canonical flat"},
};
constexpr int kP2PFormCount = (int)(sizeof(kP2PForms) / sizeof(kP2PForms[0]));

// ---- geometry: fixed latency (p2p.hip) -----------------------------------------------------------

// dwords of one ring cell: the state's F fields and the checksum, padded to whole 16-byte pieces
GGRS_HD constexpr int cell_dwords(int p) { return (state_fields(p) + 1 + 3) & ~3; }

// p2p_kernel: input rows of a stage of calls in the block's LDS
constexpr int kP2PRows = 64;
constexpr int kP2PBlock = 256;

constexpr int kFlatBlock = 64;
// rows per stage: a wave's steps in a stage are its slowest session's, so fewer, longer stages
// cost less (128 rows: one stage per 64-call launch at back = 6)
constexpr int kFlatRows = 128;
// with the LDS ring: 12 KB of rows (96 at two players: a 64-call launch is one stage) beside a
// ring of at most 28 KB per block, four blocks per CU in 160 KB
GGRS_HD constexpr int flat_rows_lds(int p) { return 12 * 1024 / (kFlatBlock * padded_players(p)); }
template <int P>
constexpr int flat_rows_lds() {
  return flat_rows_lds(P);
}

constexpr int kChainLdsRows = 16 * 1024;  // bytes of staged input rows per block
constexpr int kStashEntry = 32;  // bytes per (session, player) entry of a stash slot: 5 fields
constexpr int kChainFastLds = 40 * 1024;  // the kD form's LDS budget per block (four blocks per CU)

constexpr int kLdsPerCu = 160 * 1024;

// ---- geometry: scheduled arrivals (p2p_sched.hip) ------------------------------------------------

constexpr int kBlock = 64;

GGRS_HD inline uint32_t align16(uint32_t x) { return (x + 15) & ~15u; }
GGRS_HD inline int input_word_bytes(int P) { return P <= 1 ? 1 : (P == 2 ? 2 : 4); }

// The block's LDS (dynamic): its 64 sessions' rings [R][PC][64] uint4 (+ frame tags [R][64] with
// sparse saving; without it every frame 0 .. last save has been saved, so a cell's frame is the
// newest one <= the last save in its slot), local queues [WL][64], and per stage of K calls the
// calls' records [K][64] (u32, sparse saving u64) and the input rows [B + K][64] of frames / calls
// [stage start - B, stage end) with their row tags.
struct SchedLds {
  uint32_t o_tags, o_lq, o_arr, o_rowtag, o_rows, total;  // byte offsets (32-bit: scalar registers are scarce)
  uint32_t rec_b, rowtag_b, rows_b;                       // bytes of one stage buffer of each
};
// nbuf: stage buffers (records, row tags, rows): 2 when the control pass of stage i + 1 runs on a
// second wave beside stage i's step loop
GGRS_HD inline SchedLds sched_lds(int P, int R, int sparse, int WL, int K, int B, int nbuf = 1) {
  SchedLds l;
  const uint32_t ring = (uint32_t)R * (cell_dwords(P) / 4) * kBlock * 16;
  l.o_tags = ring;
  l.o_lq = align16(l.o_tags + (sparse ? (uint32_t)R * kBlock * 4 : 0u));
  l.o_arr = align16(l.o_lq + (uint32_t)WL * kBlock * input_word_bytes(P));
  l.rec_b = align16((uint32_t)K * kBlock * (sparse ? 8 : 4));  // the calls' records
  l.o_rowtag = l.o_arr + (uint32_t)nbuf * l.rec_b;
  l.rowtag_b = align16((uint32_t)(K + B) * 4);
  l.o_rows = l.o_rowtag + (uint32_t)nbuf * l.rowtag_b;
  l.rows_b = align16((uint32_t)(K + B) * kBlock * input_word_bytes(P));
  l.total = l.o_rows + (uint32_t)nbuf * l.rows_b;
  return l;
}

// the time-aligned form (p2p_sched_chains_kernel)
constexpr int kCS = 16;          // sessions per block
constexpr int kSL = 16;          // lanes per session: slot 0 the lineage, slots 1..15 chains
constexpr int kChainThreads = kCS * kSL + 64;  // four step waves + the control wave
constexpr int kMaxChainDepth = 12;              // max_prediction of the time-aligned form
constexpr int kChainMaxK = 32;                  // calls per stage (the control wave's prefetch registers)
constexpr int kChainMaxCalls = 2000;  // calls per launch: chain keys (ranks) << 4 | slot fit 15 bits

// per (frame % TW, session): two uint4
//   e0.x  the delivered frame of the call at this current frame that advances (the last one there)
//   e0.y  bit 0 a call has this current frame | 1 it advances | 2-5 its disconnect mask
//   e0.zw chain 0 starting here: delivered frame, flags (bit 0 valid | 4-7 slot | 8-11 depth |
//         12-15 disconnect mask | 16-31 key)
//   e1.xy chain 1 (a second chain starting at the same frame), e1.z the local players' input
struct ChainLds {
  uint32_t o_tab, o_rowtag, o_rows, o_arr, o_ev, o_range, o_lf, total;
  uint32_t rowtag_b, rows_b, arr_b, ev_b;
};
GGRS_HD inline ChainLds chain_lds(int P, int R, int TW, int K, int B) {
  ChainLds l;
  l.o_tab = (uint32_t)R * (cell_dwords(P) / 4) * kCS * 16;
  l.rowtag_b = align16((uint32_t)(K + B) * 4);
  l.rows_b = align16((uint32_t)(K + B) * kCS * input_word_bytes(P));
  l.arr_b = align16((uint32_t)K * kCS * 4);
  l.ev_b = align16((uint32_t)K * kCS);
  l.o_rowtag = l.o_tab + (uint32_t)TW * kCS * 32;
  l.o_rows = l.o_rowtag + 3 * l.rowtag_b;  // three stage buffers: the control's, the steps', the prefetch's
  l.o_arr = l.o_rows + 3 * l.rows_b;
  l.o_ev = l.o_arr + 2 * l.arr_b;
  l.o_range = l.o_ev + 2 * l.ev_b;
  l.o_lf = l.o_range + 2 * kCS * 8;
  l.total = l.o_lf + kCS * 4 * 4;
  return l;
}

// ---- the compile-time local mask -----------------------------------------------------------------

// Two players, one of them local (the usual peer): the kernels take the local mask as the template
// argument kLocal = 1 or 2; -1 reads it from the parameters.
constexpr int p2p_local_spec(int players, uint32_t local_mask) {
  return players == 2 && (local_mask == 1u || local_mask == 2u) ? (int)local_mask : -1;
}

// ---- fixed latency: the next launch --------------------------------------------------------------

struct P2PPlanIn {
  int64_t sessions;
  int32_t players;
  uint32_t local_mask;
  int32_t remote_latency, input_delay, max_prediction;
  int32_t R, cap;  // ring cells per session, input rows
  int32_t predictor;
  bool sparse;     // sparse saving
  bool trace;      // a display trace is kept
  bool desync;     // desync detection is on
  bool dbg_armed;  // a debug flip is armed now
  bool dbg_ever;   // ... or was once: the states may no longer be the canonical ones
  P2PForm form;
  int32_t num_cus;
  int32_t f0, left;  // the next call, and how many this advance still runs
  int32_t row_left;  // calls left of the row-budget piece the chains form is in (P2PLaunch::row_left
                     // of the advance's previous launch; 0 at its start)
};

enum class P2PKernel : int32_t {
  kLockstep,     // p2p_lockstep_kernel<P> (max_prediction 0)
  kUnstaged,     // p2p_kernel<P, false>
  kStaged,       // p2p_kernel<P, true>
  kFlat,         // p2p_flat_kernel<P, kLocal, plain, sparse, lds_ring>
  kCanon,        // p2p_canon_kernel<P, kLocal>
  kCanonSparse,  // p2p_canon_sparse_kernel<P, kLocal>
  kChains,       // p2p_chains_kernel<P, chain_batch, chain_fast ? 8 : 0>
};
constexpr const char* kP2PKernelNames[] = {"lockstep", "p2p_kernel", "p2p_kernel", "flat", "canon", "canon_sparse", "chains"};

struct P2PLaunch {
  P2PKernel kernel;
  int32_t kLocal;  // 1, 2 or -1
  bool plain, sparse, lds_ring;  // flat
  bool chain_batch, chain_fast;  // chains
  int32_t spw;                   // chains: sessions per block (one wave)
  uint32_t grid, block;
  size_t lds;  // dynamic LDS bytes
  int32_t n;   // calls this launch runs
  int32_t row_left;
};

// The launch that runs the next calls of an advance.  GGRS_OK, or the error code with its message in *msg.
inline int p2p_plan_next(const P2PPlanIn& in, P2PLaunch* out, const char** msg) {
  const int64_t S = in.sessions;
  const int P = in.players;
  const int32_t D = in.remote_latency, delay = in.input_delay;
  P2PLaunch L{};
  L.kLocal = -1;
  L.n = in.left;
  if (in.max_prediction == 0) {  // lockstep mode: one thread per session applies the host's replay
    L.kernel = P2PKernel::kLockstep;
    L.grid = (uint32_t)grid_of(S, 256);
    L.block = 256;
    *out = L;
    return GGRS_OK;
  }
  // the chains form: forced, or by default when the flat kernel's one thread per session would
  // leave most SIMDs idle.  Its lanes per session: D roles + the batch for 2 <= D <= 8, else D + 1 roles
  const bool chain_batch = D >= 2 && D <= 8;
  const int G = (chain_batch ? D : D + 1) * padded_players(P);
  // plain history: the session's states are the canonical ones the remote inputs determine (the
  // canonical flat kernel also keeps the desync history; the chains form does not)
  const bool plain_hist = !in.sparse && !in.trace && !in.dbg_ever;
  const bool chains_ok = plain_hist && !in.desync && G <= kWave &&
                         (uint64_t)S * in.R * cell_dwords(P) * 4 < ((uint64_t)1 << 30);
  if (in.form == P2PForm::kChains && !chains_ok) {
    *msg = "the chains form needs plain launches (no desync detection, trace, debug flip or "
           "sparse saving), (remote_latency + 1) x padded players <= 64 lanes and a ring < 1 GiB";
    return GGRS_E_STATE;
  }
  bool chains = chains_ok && (in.form == P2PForm::kChains ||
                              (in.form == P2PForm::kDefault && grid_of(S, kFlatBlock) <= in.num_cus));
  // the canonical flat kernel needs the same plain history, and its sparse-saving form the same
  // launches with sparse saving on
  const bool pick = in.form == P2PForm::kDefault || in.form == P2PForm::kCanon;
  bool canon = plain_hist && pick;
  bool canon_sparse = in.sparse && !in.trace && !in.dbg_ever && pick;
  // all three need the remote inputs flowing: the calls before that (f0 < D) run as kFlatQueues
  P2PForm form = in.form;
  if ((chains || canon || canon_sparse) && in.f0 < D) {
    L.n = std::min(in.left, D - in.f0);
    form = P2PForm::kFlatQueues;
    chains = canon = canon_sparse = false;
  }
  if (chains) {
    const int spw = kWave / G;
    const int row_bytes = spw * padded_players(P);
    // a launch's rows (f0 - 2D - delay .. f0 + n - 1) must fit the block's LDS: longer runs split
    const int32_t max_n = kChainLdsRows / row_bytes - 2 * D - delay;
    if (max_n < 1) {
      *msg = "remote_latency / input_delay too large for the chains form";
      return GGRS_E_INVALID;
    }
    const int32_t piece = in.row_left > 0 ? in.row_left : std::min(in.left, max_n);
    // config 2's P2P shape (latency 8, two players): the compile-time form, whose decoded input
    // records cap a launch's rows by its LDS budget, so it splits a row-budget piece further
    const size_t fast_fixed = (size_t)2 * 8 * row_bytes * kStashEntry + 16 + 16;  // stash, alignment, input-0 record
    const int32_t fast_n = (int32_t)((kChainFastLds - fast_fixed) / ((size_t)row_bytes * 17)) - 2 * D - delay;
    // (an input delay so long that no call fits the budget: the general form)
    const bool fast = chain_batch && D == 8 && P == 2 && fast_n >= 1;
    L.n = fast ? std::min(piece, fast_n) : piece;
    L.row_left = piece - L.n;
    size_t lds = (size_t)(L.n + 2 * D + delay) * row_bytes;
    const size_t n_entries = lds;
    if (chain_batch) lds = ((lds + 15) & ~(size_t)15) + (size_t)(D + 1) * kWave * kStashEntry;
    if (fast)  // rows, the stash's 2D slots of row_bytes entries, the input records
      lds = ((n_entries + 15) & ~(size_t)15) + (size_t)2 * D * row_bytes * kStashEntry + (n_entries + 1) * 16;
    L.kernel = P2PKernel::kChains;
    L.chain_batch = chain_batch;
    L.chain_fast = fast;
    L.spw = spw;
    L.grid = (uint32_t)grid_of(S, spw);
    L.block = kWave;
    L.lds = lds;
    *out = L;
    return GGRS_OK;
  }
  // stage input rows in LDS unless a call reaches further back than a stage holds
  const int32_t back = (in.sparse ? in.R - 1 : D) + delay;
  const bool staged = back + 1 <= kP2PRows - 1 && form != P2PForm::kUnstaged;
  // the flat form by default: with the session-major ring its saves stay whole cache lines
  // whatever frame each lane is at
  const bool flat = staged && form != P2PForm::kLockstep && form != P2PForm::kChains;
  if (!flat) {
    L.kernel = staged ? P2PKernel::kStaged : P2PKernel::kUnstaged;
    L.grid = (uint32_t)grid_of(S, kP2PBlock);
    L.block = kP2PBlock;
    *out = L;
    return GGRS_OK;
  }
  L.grid = (uint32_t)grid_of(S, kFlatBlock);
  L.block = kFlatBlock;
  // the LDS ring when a stage of rows holds a call's reach and the block's rings fit: 28 KB
  // (four blocks, one per SIMD, in a CU's 160 KB beside 12 KB of rows each), or more when the
  // grid puts fewer blocks on each CU (config 2's P2P shape: 4096 sessions = 64 blocks, R = 10:
  // 30 KB of rings)
  const size_t ring_lds = (size_t)in.R * (cell_dwords(P) / 4) * kFlatBlock * 16;
  const size_t rows_lds = (size_t)flat_rows_lds(P) * kFlatBlock * padded_players(P);
  const int64_t per_cu = ((int64_t)L.grid + in.num_cus - 1) / in.num_cus;
  const bool fits = ring_lds <= 28 * 1024 ||
                    (ring_lds + rows_lds <= 64 * 1024 && per_cu * (int64_t)(ring_lds + rows_lds) <= kLdsPerCu);
  const bool lds_ring = form != P2PForm::kFlatHbm && fits && back + 1 <= flat_rows_lds(P) - 1;
  L.lds = lds_ring ? ring_lds : 0;
  if (lds_ring && (canon || canon_sparse)) {
    L.kernel = canon_sparse ? P2PKernel::kCanonSparse : P2PKernel::kCanon;
    L.kLocal = p2p_local_spec(P, in.local_mask);
  } else {
    L.kernel = P2PKernel::kFlat;
    L.plain = !in.desync && !in.trace && !in.dbg_armed;
    L.sparse = in.sparse;
    L.lds_ring = lds_ring;
    L.kLocal = in.sparse ? -1 : p2p_local_spec(P, in.local_mask);  // (the sparse form is not specialised)
  }
  *out = L;
  return GGRS_OK;
}

// ---- scheduled arrivals: the next launch ---------------------------------------------------------

// GGRS_SCHED_SPLIT, GGRS_SCHED_CHAINS, GGRS_SCHED_K: read at every advance, so they take effect on
// an engine that already exists
struct SchedOverrides {
  bool split_off = false;  // GGRS_SCHED_SPLIT=0: never the two-wave form
  int chains = -1;         // GGRS_SCHED_CHAINS: 0 never the time-aligned form, 1 at any session count
  int K = 16;              // GGRS_SCHED_K: the time-aligned form's calls per stage (clamped)
};
inline SchedOverrides sched_overrides_from_env() {
  SchedOverrides o;
  if (const char* s = getenv("GGRS_SCHED_SPLIT")) o.split_off = s[0] == '0';
  if (const char* s = getenv("GGRS_SCHED_CHAINS")) o.chains = s[0] == '0' ? 0 : (s[0] == '1' ? 1 : -1);
  if (const char* s = getenv("GGRS_SCHED_K")) o.K = atoi(s);
  return o;
}

struct SchedPlanIn {
  int64_t sessions;
  int32_t players;
  uint32_t local_mask;
  int32_t input_delay, max_prediction;
  int32_t R, cap;
  int32_t predictor;
  bool sparse, desync, peer_reports, trace;
  int32_t num_cus;
  int32_t left;      // calls this advance still runs
  int32_t cap_left;  // calls left of the capacity piece the advance is in (SchedLaunch::cap_left of
                     // its previous launch; 0 at its start)
};

struct SchedLaunch {
  bool chains;  // p2p_sched_chains_kernel<P, predictor, kLocal, feat>,
                // else p2p_sched_kernel<P, sparse, predictor, kLocal, split, feat>
  bool split;   // two waves per block: the control pass of the next stage beside the step loop
  bool feat;    // desync detection, peer reports and the display trace compiled in
  int32_t kLocal;
  int32_t K, B, WL, TW;  // SchedParams
  int32_t nbuf;          // stage buffers of the one-thread-per-session form
  uint32_t grid, block;
  size_t lds;
  int32_t n;
  int32_t cap_left;
};

inline int sched_plan_next(const SchedPlanIn& in, const SchedOverrides& ov, SchedLaunch* out, const char** msg) {
  const int P = in.players;
  SchedLaunch L{};
  // a launch reads at most cap calls' arrival rows
  const int32_t piece = in.cap_left > 0 ? in.cap_left : std::min(in.left, in.cap);
  // stage geometry: B rows behind a stage's first call (a rollback's confirmed inputs reach back
  // max_prediction frames, a burst after a stall a few more), K calls per stage as many as keep the
  // block's LDS within its share of the CU -- at least 8
  int WL = 2;
  while (WL < in.max_prediction + in.input_delay + 2) WL *= 2;
  const int B = 2 * in.max_prediction + 4;
  // the LDS a block may take without costing residency: 160 KB per CU shared by the blocks each CU
  // must hold at once (65,536 sessions: four, one per SIMD -> 40 KB; 4,096 sessions: one -> all of it)
  const int64_t blocks = grid_of(in.sessions, kBlock);
  const int64_t per_cu = std::max<int64_t>(1, std::min<int64_t>(4, (blocks + in.num_cus - 1) / in.num_cus));
  const uint32_t budget = (uint32_t)(kLdsPerCu / per_cu) - 1024;
  // Two waves per block (the control pass of the next stage beside the step loop) when each CU holds
  // one block: its second wave runs on a SIMD that would idle
  const bool split = !in.sparse && per_cu == 1 && blocks <= in.num_cus && !ov.split_off;
  const int nbuf = split ? 2 : 1;
  // (the two-wave form overlaps all but the first stage's control pass, but shorter stages cost the
  // step wave more than they hide: 4,096 sessions 180 / 170 / 158 / 156 / 156 us at 8 / 12 / 16 / 24
  // / 42 calls per stage, profiles/r05ak_k*)
  // and at most 64 - B, so that a stage's rows fit the control pass's 64-bit change masks (its fast form)
  int K = std::max(8, std::min(64, 64 - B));
  while (K > 8 && sched_lds(P, in.R, in.sparse, WL, K, B, nbuf).total > budget) K -= 4;
  const size_t shm = sched_lds(P, in.R, in.sparse, WL, K, B, nbuf).total;
  if (shm > (size_t)kLdsPerCu) {
    *msg = "max_prediction too large for the scheduled kernel's LDS";
    return GGRS_E_INVALID;
  }
  // desync detection, peer reports or the display trace: the kernels with their code (a session's
  // standing reports can only come from an engine given reports)
  const bool feat = in.desync || in.peer_reports || in.trace;
  L.B = B;
  L.WL = WL;
  L.kLocal = in.predictor == 0 && !in.sparse ? p2p_local_spec(P, in.local_mask) : -1;
  // The time-aligned form (a session's replays on 16 lanes) for few sessions: when its blocks of 16
  // sessions fill at most two per CU (lockstep mode, sparse saving, peer reports and the display
  // trace take the one-thread-per-session form)
  int remote = 0;
  for (int k = 0; k < P; k++) remote += !((in.local_mask >> k) & 1);
  const int64_t cblocks = grid_of(in.sessions, kCS);
  const bool chains = !in.sparse && in.max_prediction >= 1 && in.max_prediction <= kMaxChainDepth && remote <= 2 &&
                      !in.peer_reports && !in.trace && ov.chains != 0 &&
                      (cblocks <= 2 * (int64_t)in.num_cus || ov.chains == 1);
  if (chains) {
    L.n = std::min(piece, kChainMaxCalls);  // (its chain keys)
    // K calls per stage: the step waves trail the control wave by a stage, so shorter stages overlap
    // more of the two; the tables hold the frames of two stages + max_prediction + the delay
    const int Kc = std::max(4, std::min(std::min(ov.K, 64 - B), kChainMaxK));
    int TW = 16;
    while (TW < 2 * Kc + in.max_prediction + in.input_delay + 8) TW *= 2;
    const ChainLds cl = chain_lds(P, in.R, TW, Kc, B);
    if (cl.total > (uint32_t)kLdsPerCu) {
      *msg = "input_delay too large for the scheduled kernel's LDS";
      return GGRS_E_INVALID;
    }
    L.chains = true;
    L.feat = feat;
    L.K = Kc;
    L.TW = TW;
    L.grid = (uint32_t)cblocks;
    L.block = kChainThreads;
    L.lds = cl.total;
  } else {
    L.n = piece;
    L.split = split;
    L.feat = feat || in.sparse;  // (sparse saving keeps the features compiled in)
    L.K = K;
    L.nbuf = nbuf;
    L.grid = (uint32_t)grid_of(in.sessions, kBlock);
    L.block = split ? 2 * kBlock : kBlock;
    L.lds = shm;
  }
  L.cap_left = piece - L.n;
  *out = L;
  return GGRS_OK;
}

}  // namespace ggrs
