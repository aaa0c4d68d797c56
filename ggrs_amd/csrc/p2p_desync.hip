// p2p_desync.hip -- the receive side of desync detection of the any-network P2P engine (p2p_sched.hip,
// p2p_ingest.hip, p2p_emit.hip, p2p_time_sync.hip): every session's GgrsEvent::DesyncDetected on the
// device.  The scheduled kernels run check_checksum_send_interval and leave the call's report row
// (rep_frame, rep_ck, rep_lconf, rep_ll); this unit is UdpProtocol::on_checksum_report
// (src/network/protocol.rs:663-682) and compare_local_checksums_against_peers
// (src/sessions/p2p_session.rs:904-937) with the history push of check_checksum_send_interval
// (:965-970), for one endpoint per session holding all of its remote players (packet emit's
// simplification), in the order of ggrs_amd/desync.py's SchedDesyncDetector.poll.
//
// Per session: local_checksum_history and pending_checksums, at most MAX_CHECKSUM_HISTORY_SIZE = 32
// (frame, u16 checksum) entries each, both empty; a cursor into the peer's report rows; the newest
// frame received from the peer; last_recv; a status word; the summary.  Call c, after it ran:
//   1. delivery: the peer's rows g = cursor, cursor + 1, .. while g < c and the peer's last queued
//      frame after its call g (the inputs the report travelled with) <= last_recv -- the feed's ack row,
//      else the running maximum of the arrival rows, as the emits and time sync derive it.  A row with
//      frame >= 0 is on_checksum_report: with 32 entries pending, those with frame < f - 31 interval
//      go first; then the row is inserted.
//      Stated divergence: a report whose frame is not a positive multiple of the interval, or not above
//      the newest frame already received, is refused and counted (the reference accepts any frame; a
//      peer of the same configuration sends none).  So the table never exceeds 32 entries: at most 31
//      distinct multiples lie in [f - 31 interval, f).
//   2. the local report: rep_frame[c] >= 0 enters the history with rep_ck[c]; a 33rd entry prunes it
//      to frame >= f - 31 interval (the engine's reports are consecutive multiples: the oldest goes).
//   3. compare: every pending report in ascending frame order; one with frame < rep_lconf[c] and its
//      frame in the history is compared and removed; a difference is a DesyncDetected (call, session,
//      frame, local checksum, remote checksum).
//   4. a session whose cursor is more than input_capacity rows behind the rows added when a launch
//      starts has lost the row at its cursor to the ring: GGRS_DESYNC_ROW_LOST, sticky, no step from
//      the launch's first call on.
// Reports arrive in ascending frame order (the refusal rule), local reports are sent in it, so both
// tables are insertion-ordered and frame-ordered at once: no sort, a prune drops a prefix, the
// comparison walks the two tables as a merge.
//
// One thread per session, one wave per block; the launch's calls are walked in order.  The tables live
// in HBM, [2][32][S] frames and checksums; kLds (the default): the block's tables sit in LDS for the
// launch (24 KB) and go back at its end, else every access is to HBM.  A group of calls' words is
// loaded before its first use; the peer's row at the cursor is held in registers, loaded when the
// cursor moves (lanes mostly share g: coalesced), and the first pending frame too, so a call that
// delivers nothing and compares nothing touches no table.  Events go to the event list through one
// atomic per wave and compare step (ballot + popcount); the counter stays exact when the list is full.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdlib>
#include <vector>

#include "common.h"
#include "emit_device.h"
#include "p2p_engine.h"

using namespace ggrs;

namespace {

constexpr int32_t kNull = GGRS_NULL_FRAME;
constexpr int kDcBlock = kEmitBlock;
constexpr int kDcGroup = kEmitGroup;
constexpr int32_t kDcMaxEvents = 1 << 26;
static_assert(kDcBlock == 64, "one wave per block: the event append ballots the block");

struct DcParams {
  int64_t S;
  int32_t cap, c0, n;
  int32_t pkt, interval, max_events, added;
  const int32_t* rep_frame;    // [cap][S] the local report rows
  const uint16_t* rep_ck;
  const int32_t* rep_lconf;
  const int32_t* arrive;       // [cap][S] (the packet feed off)
  const int32_t* pkt_ack;      // [cap][S] (the packet feed on)
  const int32_t* peer_frame;   // [cap][S] the peer's report rows
  const uint16_t* peer_ck;
  const int32_t* peer_ll;
  int32_t* frames;             // [2][kDcTable][S]
  uint16_t* cks;               // [2][kDcTable][S]
  int32_t* st;                 // [kDcFields][S]
  int32_t* events;             // [4][max_events]
  unsigned long long* count;
};

template <bool kLds>
__global__ __launch_bounds__(kDcBlock) void p2p_desync_kernel(DcParams p) {
  __shared__ int32_t s_f[kLds ? 2 * kDcTable * kDcBlock : 1];
  __shared__ uint16_t s_c[kLds ? 2 * kDcTable * kDcBlock : 1];
  const int t = threadIdx.x;
  const int64_t S = p.S;
  const int64_t s0 = (int64_t)blockIdx.x * kDcBlock;
  const int nb = (int)min((int64_t)kDcBlock, S - s0);
  const bool live = t < nb;
  const int64_t s = live ? s0 + t : s0;  // idle lanes shadow the block's first session, never store
  const int32_t cap = p.cap, I = p.interval;
  auto fld = [&](int f) -> int32_t& { return p.st[(int64_t)f * S + s]; };
  // entry i of table T (0 the history, 1 the pending reports): column t is this thread's own
  auto F = [&](int T, int i) -> int32_t& {
    if constexpr (kLds) return s_f[(T * kDcTable + i) * kDcBlock + t];
    else return p.frames[(int64_t)(T * kDcTable + i) * S + s];
  };
  auto C = [&](int T, int i) -> uint16_t& {
    if constexpr (kLds) return s_c[(T * kDcTable + i) * kDcBlock + t];
    else return p.cks[(int64_t)(T * kDcTable + i) * S + s];
  };
  int32_t cursor = fld(kDcCursor), newest = fld(kDcNewest), recv = fld(kDcRecv), status = fld(kDcStatus);
  int32_t hn = fld(kDcHist), pn = fld(kDcPend), refused = fld(kDcRefused), nev = fld(kDcEvents);
  int32_t first_call = fld(kDcFirstCall), first_frame = fld(kDcFirstFrame), first_local = fld(kDcFirstLocal),
          first_remote = fld(kDcFirstRemote);
  if (kLds) {
#pragma unroll
    for (int i = 0; i < kDcTable; i++) {
      if (i < hn) {
        s_f[i * kDcBlock + t] = p.frames[(int64_t)i * S + s];
        s_c[i * kDcBlock + t] = p.cks[(int64_t)i * S + s];
      }
      if (i < pn) {
        s_f[(kDcTable + i) * kDcBlock + t] = p.frames[(int64_t)(kDcTable + i) * S + s];
        s_c[(kDcTable + i) * kDcBlock + t] = p.cks[(int64_t)(kDcTable + i) * S + s];
      }
    }
  }
  // 4. the ring holds the peer's rows added - cap .. added - 1
  if (status == 0 && p.added - cursor > cap) status = GGRS_DESYNC_ROW_LOST;
  const bool run = live && status == 0;
  // the peer's row at the cursor (this launch reads rows up to c0 + n - 2, all of them added)
  const int32_t glast = p.c0 + p.n - 2;
  int32_t nx_frame = kNull, nx_ll = 0;
  uint32_t nx_ck = 0;
  bool nx_ok = false;
  auto load_next = [&]() {
    nx_ok = run && cursor <= glast;
    if (nx_ok) {
      const int64_t o = (int64_t)(cursor % cap) * S + s;
      nx_frame = p.peer_frame[o];
      nx_ck = p.peer_ck[o];
      nx_ll = p.peer_ll[o];
    }
  };
  load_next();
  int32_t pf0 = run && pn > 0 ? (int32_t)F(1, 0) : INT32_MAX;  // the first pending frame

  for (int32_t k0 = 0; k0 < p.n; k0 += kDcGroup) {
    const int gn = min(kDcGroup, p.n - k0);
    // the group's per-call words, all loads in flight together (a short group repeats its last call)
    int32_t rf8[kDcGroup], lc8[kDcGroup], rcv8[kDcGroup];
    uint32_t ck8[kDcGroup];
#pragma unroll
    for (int g = 0; g < kDcGroup; g++) {
      const int64_t o = (int64_t)((p.c0 + k0 + min(g, gn - 1)) % cap) * S + s;
      rf8[g] = p.rep_frame[o];
      ck8[g] = p.rep_ck[o];
      lc8[g] = p.rep_lconf[o];
      rcv8[g] = p.pkt ? p.pkt_ack[o] : p.arrive[o];
    }
    for (int g = 0; g < gn; g++) {
      const int32_t c = p.c0 + k0 + g;
      // this call's words: the front of the batch, which shifts down a call per iteration (indexing it by
      // g would put it in scratch memory)
      const int32_t rf = rf8[0], lconf = lc8[0], rcv = rcv8[0];
      const uint32_t rck = ck8[0];
#pragma unroll
      for (int j = 0; j < kDcGroup - 1; j++) {
        rf8[j] = rf8[j + 1];
        ck8[j] = ck8[j + 1];
        lc8[j] = lc8[j + 1];
        rcv8[j] = rcv8[j + 1];
      }
      recv = p.pkt ? rcv : max(recv, rcv);
      // 1. on_checksum_report (protocol.rs:663-682) for the rows this call's poll delivers
      while (true) {
        const bool take = nx_ok && cursor < c && nx_ll <= recv;
        if (!__any(take)) break;
        if (take) {
          const int32_t f = nx_frame;
          if (f >= 0) {
            if (f == 0 || f % I != 0 || f <= newest) {
              ++refused;
            } else {
              if (pn >= kDcTable) {
                const int32_t oldest = f - (kDcTable - 1) * I;
                int k = 0;
                while (k < pn && F(1, k) < oldest) ++k;
                if (k == 0) k = 1;  // (never: at most 31 multiples lie in [oldest, f))
                for (int j = k; j < pn; j++) {
                  F(1, j - k) = F(1, j);
                  C(1, j - k) = C(1, j);
                }
                pn -= k;
                pf0 = pn > 0 ? (int32_t)F(1, 0) : INT32_MAX;
              }
              F(1, pn) = f;
              C(1, pn) = (uint16_t)nx_ck;
              if (pn == 0) pf0 = f;
              ++pn;
              newest = f;
            }
          }
          ++cursor;
          load_next();
        }
      }
      // 2. check_checksum_send_interval's history push (p2p_session.rs:965-970)
      if (run && rf >= 0) {
        if (hn >= kDcTable) {
          const int32_t oldest = rf - (kDcTable - 1) * I;
          int k = 0;
          while (k < hn && F(0, k) < oldest) ++k;
          if (k == 0) k = 1;  // (never: the engine's reports are consecutive multiples)
          for (int j = k; j < hn; j++) {
            F(0, j - k) = F(0, j);
            C(0, j - k) = C(0, j);
          }
          hn -= k;
        }
        F(0, hn) = rf;
        C(0, hn) = (uint16_t)rck;
        ++hn;
      }
      // 3. compare_local_checksums_against_peers (:904-937): a merge of the two frame-ordered tables
      const bool go = run && pf0 < lconf;
      if (__any(go)) {
        const int n0 = go ? pn : 0;
        int i = 0, w = 0, h = 0;
        while (__any(i < n0)) {
          bool diff = false;
          int32_t f = 0;
          uint32_t remote = 0, local = 0;
          if (i < n0) {
            f = F(1, i);
            remote = C(1, i);
            bool hit = false;
            if (f < lconf) {
              while (h < hn && F(0, h) < f) ++h;
              if (h < hn && F(0, h) == f) {
                hit = true;
                local = C(0, h);
              }
            }
            if (hit) {
              diff = local != remote;
            } else {
              if (w != i) {
                F(1, w) = f;
                C(1, w) = (uint16_t)remote;
              }
              ++w;
            }
            ++i;
          }
          // the wave's events of this step: one atomic for all of them
          const unsigned long long m = __ballot(diff);
          if (m) {
            const int leader = __ffsll((long long)m) - 1;
            unsigned int lo = 0, hi = 0;
            if (t == leader) {
              const unsigned long long b = atomicAdd(p.count, (unsigned long long)__popcll(m));
              lo = (unsigned int)b;
              hi = (unsigned int)(b >> 32);
            }
            lo = __shfl(lo, leader);
            hi = __shfl(hi, leader);
            if (diff) {
              const unsigned long long at =
                  ((unsigned long long)hi << 32 | lo) + (unsigned long long)__popcll(m & ((1ull << t) - 1ull));
              if (at < (unsigned long long)p.max_events) {
                const int64_t me = p.max_events;
                p.events[at] = c;
                p.events[me + at] = (int32_t)s;
                p.events[2 * me + at] = f;
                p.events[3 * me + at] = (int32_t)(local | remote << 16);
              }
              if (nev == 0) {
                first_call = c;
                first_frame = f;
                first_local = (int32_t)local;
                first_remote = (int32_t)remote;
              }
              ++nev;
            }
          }
        }
        if (go) {
          pn = w;
          pf0 = pn > 0 ? (int32_t)F(1, 0) : INT32_MAX;
        }
      }
    }
  }
  if (live) {
    fld(kDcCursor) = cursor;
    fld(kDcNewest) = newest;
    fld(kDcRecv) = recv;
    fld(kDcStatus) = status;
    fld(kDcHist) = hn;
    fld(kDcPend) = pn;
    fld(kDcRefused) = refused;
    fld(kDcEvents) = nev;
    fld(kDcFirstCall) = first_call;
    fld(kDcFirstFrame) = first_frame;
    fld(kDcFirstLocal) = first_local;
    fld(kDcFirstRemote) = first_remote;
    if (kLds) {
#pragma unroll
      for (int i = 0; i < kDcTable; i++) {
        if (i < hn) {
          p.frames[(int64_t)i * S + s] = s_f[i * kDcBlock + t];
          p.cks[(int64_t)i * S + s] = s_c[i * kDcBlock + t];
        }
        if (i < pn) {
          p.frames[(int64_t)(kDcTable + i) * S + s] = s_f[(kDcTable + i) * kDcBlock + t];
          p.cks[(int64_t)(kDcTable + i) * S + s] = s_c[(kDcTable + i) * kDcBlock + t];
        }
      }
    }
  }
}

// GGRS_DESYNC_COMPARE_LDS=0 touches the two tables in HBM instead of holding the block's tables in LDS
// for the launch (for the comparison; default 1, which measured 7.80 against 8.54 us per call of 65,536
// sessions at interval 10 and the same 25.1 at interval 1, profiles/desync_compare_rate.json)
bool dc_lds_from_env() {
  const char* v = std::getenv("GGRS_DESYNC_COMPARE_LDS");
  return !(v && v[0] == '0');
}

int dc_need(ggrs_p2p_engine_t* e) {
  if (!e) return set_error(GGRS_E_INVALID, "null engine");
  if (!e->sched || !e->dcmp.on || e->desync_interval != e->dcmp_interval)
    return set_error(GGRS_E_STATE, "the checksum comparison needs ggrs_p2p_set_desync_compare");
  return GGRS_OK;
}

// n rows of a [.][S] table into the ring's slots from call `first` on (rows wrap at cap)
template <typename T>
int dc_ring_copy(T* ring, const T* src, int32_t first, int32_t n, int32_t cap, size_t S, hipMemcpyKind kind,
                 hipStream_t stream) {
  for (int32_t k = 0; k < n;) {
    const int32_t slot = (first + k) % cap;
    const int32_t m = std::min(n - k, cap - slot);
    HIP_TRY(hipMemcpyAsync(ring + (size_t)slot * S, src + (size_t)k * S, sizeof(T) * (size_t)m * S, kind, stream));
    k += m;
  }
  return GGRS_OK;
}

int dc_check_add(ggrs_p2p_engine_t* e, int32_t first_call, int32_t n) {
  if (n < 0 || n > e->cap) return set_error(GGRS_E_INVALID, "n_calls must be in 0..%d (input_capacity)", e->cap);
  if (first_call != e->dcmp_added)
    return set_error(GGRS_E_INVALID, "the peer's report rows are added in call order (expected call %d, got %d)",
                     e->dcmp_added, first_call);
  return GGRS_OK;
}

}  // namespace

namespace ggrs {

int p2p_desync_free(ggrs_p2p_engine* e) {
  void* bufs[] = {e->dcmp_peer_frame, e->dcmp_peer_ck, e->dcmp_peer_ll, e->dcmp_frames, e->dcmp_cks,
                  e->dcmp_st,         e->dcmp_events,  e->dcmp_count};
  for (void* b : bufs)
    if (b) (void)hipFree(b);
  e->dcmp_peer_frame = nullptr;
  e->dcmp_peer_ck = nullptr;
  e->dcmp_peer_ll = nullptr;
  e->dcmp_frames = nullptr;
  e->dcmp_cks = nullptr;
  e->dcmp_st = nullptr;
  e->dcmp_events = nullptr;
  e->dcmp_count = nullptr;
  for (hipEvent_t& ev : e->dcmp_sync) {
    if (ev) (void)hipEventDestroy(ev);
    ev = nullptr;
  }
  e->dcmp.release();
  return GGRS_OK;
}

}  // namespace ggrs

extern "C" {

int ggrs_p2p_set_desync_compare(ggrs_p2p_engine_t* e, int32_t max_events) {
  if (!e) return set_error(GGRS_E_INVALID, "null engine");
  if (e->current_frame != 0)
    return set_error(GGRS_E_STATE,
                     "the checksum comparison is part of the session's configuration (set before the first call)");
  if (!e->sched) return set_error(GGRS_E_STATE, "the checksum comparison needs ggrs_p2p_set_arrival_schedule(e, 1)");
  if (e->desync_interval <= 0 || !e->rep_frame)
    return set_error(GGRS_E_STATE, "the checksum comparison needs ggrs_p2p_set_desync_detection(e, interval > 0)");
  if (max_events < 1 || max_events > kDcMaxEvents)
    return set_error(GGRS_E_INVALID, "max_events must be in 1..%d, got %d", kDcMaxEvents, max_events);
  HIP_TRY(hipSetDevice(e->cfg.device));
  const size_t S = (size_t)e->cfg.num_sessions, rows = (size_t)e->cap * S;
  if (!e->dcmp_st) {
    HIP_TRY(hipMalloc(&e->dcmp_peer_frame, sizeof(int32_t) * rows));
    HIP_TRY(hipMalloc(&e->dcmp_peer_ck, sizeof(uint16_t) * rows));
    HIP_TRY(hipMalloc(&e->dcmp_peer_ll, sizeof(int32_t) * rows));
    HIP_TRY(hipMalloc(&e->dcmp_frames, sizeof(int32_t) * 2 * (size_t)kDcTable * S));
    HIP_TRY(hipMalloc(&e->dcmp_cks, sizeof(uint16_t) * 2 * (size_t)kDcTable * S));
    HIP_TRY(hipMalloc(&e->dcmp_st, sizeof(int32_t) * (size_t)kDcFields * S));
    HIP_TRY(hipMalloc(&e->dcmp_count, sizeof(unsigned long long)));
    for (hipEvent_t& ev : e->dcmp_sync) HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  }
  if (e->dcmp_events && max_events != e->dcmp_max_events) {
    HIP_TRY(hipFree(e->dcmp_events));
    e->dcmp_events = nullptr;
  }
  if (!e->dcmp_events) HIP_TRY(hipMalloc(&e->dcmp_events, sizeof(int32_t) * 4 * (size_t)max_events));
  HIP_TRY(hipMemsetAsync(e->dcmp_peer_frame, 0xff, sizeof(int32_t) * rows, e->stream));  // no report
  HIP_TRY(hipMemsetAsync(e->dcmp_peer_ck, 0, sizeof(uint16_t) * rows, e->stream));
  HIP_TRY(hipMemsetAsync(e->dcmp_peer_ll, 0xff, sizeof(int32_t) * rows, e->stream));
  HIP_TRY(hipMemsetAsync(e->dcmp_frames, 0xff, sizeof(int32_t) * 2 * (size_t)kDcTable * S, e->stream));
  HIP_TRY(hipMemsetAsync(e->dcmp_cks, 0, sizeof(uint16_t) * 2 * (size_t)kDcTable * S, e->stream));
  HIP_TRY(hipMemsetAsync(e->dcmp_events, 0, sizeof(int32_t) * 4 * (size_t)max_events, e->stream));
  HIP_TRY(hipMemsetAsync(e->dcmp_count, 0, sizeof(unsigned long long), e->stream));
  // every session: both tables empty, nothing delivered, received, refused or raised
  constexpr uint32_t kZero = 1u << kDcCursor | 1u << kDcStatus | 1u << kDcHist | 1u << kDcPend | 1u << kDcRefused |
                             1u << kDcEvents | 1u << kDcFirstLocal | 1u << kDcFirstRemote;
  if (int rc = emit_fill(e->dcmp_st, S, kDcFields, kZero, e->stream)) return rc;
  HIP_TRY(hipStreamSynchronize(e->stream));
  e->dcmp.configure(0, 0);
  e->dcmp_interval = e->desync_interval;
  e->dcmp_max_events = max_events;
  e->dcmp_added = 0;
  return GGRS_OK;
}

int ggrs_p2p_add_remote_reports(ggrs_p2p_engine_t* e, int32_t first_call, int32_t n, const int32_t* frames,
                                const uint16_t* checksums, const int32_t* local_last, int32_t on_device) {
  if (int rc = dc_need(e)) return rc;
  if (int rc = dc_check_add(e, first_call, n)) return rc;
  if (n == 0) return GGRS_OK;
  if (!frames || !checksums || !local_last) return set_error(GGRS_E_INVALID, "null argument");
  HIP_TRY(hipSetDevice(e->cfg.device));
  const size_t S = (size_t)e->cfg.num_sessions;
  const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  if (int rc = dc_ring_copy(e->dcmp_peer_frame, frames, first_call, n, e->cap, S, kind, e->stream)) return rc;
  if (int rc = dc_ring_copy(e->dcmp_peer_ck, checksums, first_call, n, e->cap, S, kind, e->stream)) return rc;
  if (int rc = dc_ring_copy(e->dcmp_peer_ll, local_last, first_call, n, e->cap, S, kind, e->stream)) return rc;
  if (!on_device) HIP_TRY(hipStreamSynchronize(e->stream));  // (the caller's arrays are free again)
  e->dcmp_added = first_call + n;
  return GGRS_OK;
}

int ggrs_p2p_add_remote_reports_from(ggrs_p2p_engine_t* e, ggrs_p2p_engine_t* peer, int32_t first_call, int32_t n) {
  if (int rc = dc_need(e)) return rc;
  if (!peer || peer == e) return set_error(GGRS_E_INVALID, "the peer is another engine");
  if (!peer->sched || peer->desync_interval <= 0 || !peer->rep_frame)
    return set_error(GGRS_E_STATE, "the peer engine has report rows with arrival schedules and desync detection only");
  if (peer->cfg.num_sessions != e->cfg.num_sessions || peer->cfg.device != e->cfg.device)
    return set_error(GGRS_E_INVALID, "the peer engine must hold the same sessions on the same device");
  if (int rc = dc_check_add(e, first_call, n)) return rc;
  if ((int64_t)first_call + n > peer->current_frame || first_call < peer->current_frame - peer->cap)
    return set_error(GGRS_E_INVALID, "calls %d .. %d are not among the last %d calls the peer has run (%d run)", first_call,
                     first_call + n - 1, peer->cap, peer->current_frame);
  if (n == 0) return GGRS_OK;
  HIP_TRY(hipSetDevice(e->cfg.device));
  const size_t S = (size_t)e->cfg.num_sessions;
  // after the peer's launches that wrote the rows ...
  HIP_TRY(hipEventRecord(e->dcmp_sync[0], peer->stream));
  HIP_TRY(hipStreamWaitEvent(e->stream, e->dcmp_sync[0], 0));
  for (int32_t k = 0; k < n;) {  // both rings wrap
    const int32_t src = (first_call + k) % peer->cap;
    const int32_t m = std::min(n - k, peer->cap - src);
    const size_t off = (size_t)src * S;
    if (int rc = dc_ring_copy(e->dcmp_peer_frame, peer->rep_frame + off, first_call + k, m, e->cap, S,
                              hipMemcpyDeviceToDevice, e->stream))
      return rc;
    if (int rc = dc_ring_copy(e->dcmp_peer_ck, peer->rep_ck + off, first_call + k, m, e->cap, S, hipMemcpyDeviceToDevice,
                              e->stream))
      return rc;
    if (int rc = dc_ring_copy(e->dcmp_peer_ll, peer->rep_ll + off, first_call + k, m, e->cap, S, hipMemcpyDeviceToDevice,
                              e->stream))
      return rc;
    k += m;
  }
  // ... and before the peer's next launch overwrites them
  HIP_TRY(hipEventRecord(e->dcmp_sync[1], e->stream));
  HIP_TRY(hipStreamWaitEvent(peer->stream, e->dcmp_sync[1], 0));
  e->dcmp_added = first_call + n;
  return GGRS_OK;
}

int ggrs_p2p_compare_reports(ggrs_p2p_engine_t* e, int32_t first_call, int32_t n, int32_t* n_events_total) {
  if (int rc = dc_need(e)) return rc;
  PacketEmitState& dc = e->dcmp;
  const int32_t oldest_held = std::max(e->next_input_frame, e->next_arrival_call) - e->cap;
  if (int rc = dc.check_order(first_call, n, e->current_frame, oldest_held, e->cap, false, "reports are compared"))
    return rc;
  if (n > 0 && e->dcmp_added < first_call + n - 1)
    return set_error(GGRS_E_STATE, "the peer's report rows of call %d have not been added (calls up to %d need its rows "
                     "up to call %d)", e->dcmp_added, first_call + n - 1, first_call + n - 2);
  HIP_TRY(hipSetDevice(e->cfg.device));
  if (n > 0) {
    if (int rc = e->timer.before(e->stream)) return rc;
    const DcParams p{(int64_t)e->cfg.num_sessions, e->cap, first_call, n, e->pkt, e->dcmp_interval, e->dcmp_max_events,
                     e->dcmp_added, e->rep_frame, e->rep_ck, e->rep_lconf, e->arrive, e->feed.ack, e->dcmp_peer_frame,
                     e->dcmp_peer_ck, e->dcmp_peer_ll, e->dcmp_frames, e->dcmp_cks, e->dcmp_st, e->dcmp_events,
                     e->dcmp_count};
    const int64_t grid = grid_of(p.S, kDcBlock);
    if (dc_lds_from_env())
      p2p_desync_kernel<true><<<grid, kDcBlock, 0, e->stream>>>(p);
    else
      p2p_desync_kernel<false><<<grid, kDcBlock, 0, e->stream>>>(p);
    HIP_TRY(hipGetLastError());
    e->timer.count();
    dc.next = first_call + n;
  }
  if (n_events_total) {
    unsigned long long total = 0;
    HIP_TRY(hipMemcpyAsync(&total, e->dcmp_count, sizeof(total), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    *n_events_total = (int32_t)std::min<unsigned long long>(total, INT32_MAX);
  }
  return GGRS_OK;
}

int ggrs_p2p_read_desync_events(ggrs_p2p_engine_t* e, int32_t first, int32_t max, int32_t* call, int32_t* session,
                                int32_t* frame, uint16_t* local, uint16_t* remote, int32_t* n_read) {
  if (int rc = dc_need(e)) return rc;
  if (first < 0 || max < 0 || !n_read) return set_error(GGRS_E_INVALID, "first and max must be >= 0, n_read not null");
  HIP_TRY(hipSetDevice(e->cfg.device));
  unsigned long long total = 0;
  HIP_TRY(hipMemcpyAsync(&total, e->dcmp_count, sizeof(total), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  const int64_t kept = (int64_t)std::min<unsigned long long>(total, (unsigned long long)e->dcmp_max_events);
  const int64_t n = std::max<int64_t>(0, std::min<int64_t>(max, kept - first));
  *n_read = (int32_t)n;
  if (n == 0) return GGRS_OK;
  const size_t me = (size_t)e->dcmp_max_events;
  std::vector<int32_t> words((size_t)n);
  if (call) HIP_TRY(hipMemcpyAsync(call, e->dcmp_events + first, 4 * (size_t)n, hipMemcpyDeviceToHost, e->stream));
  if (session)
    HIP_TRY(hipMemcpyAsync(session, e->dcmp_events + me + first, 4 * (size_t)n, hipMemcpyDeviceToHost, e->stream));
  if (frame)
    HIP_TRY(hipMemcpyAsync(frame, e->dcmp_events + 2 * me + first, 4 * (size_t)n, hipMemcpyDeviceToHost, e->stream));
  const hipError_t rc =
      hipMemcpyAsync(words.data(), e->dcmp_events + 3 * me + first, 4 * (size_t)n, hipMemcpyDeviceToHost, e->stream);
  const hipError_t waited = hipStreamSynchronize(e->stream);  // (no copy may still write `words` when it is freed)
  HIP_TRY(rc);
  HIP_TRY(waited);
  for (int64_t i = 0; i < n; i++) {
    if (local) local[i] = (uint16_t)((uint32_t)words[(size_t)i] & 0xffffu);
    if (remote) remote[i] = (uint16_t)((uint32_t)words[(size_t)i] >> 16);
  }
  return GGRS_OK;
}

int ggrs_p2p_read_desync_state(ggrs_p2p_engine_t* e, int32_t* status, int32_t* n_events, int32_t* first_call,
                               int32_t* first_frame, int32_t* first_local, int32_t* first_remote, int32_t* refused,
                               int32_t* history, int32_t* pending) {
  if (int rc = dc_need(e)) return rc;
  HIP_TRY(hipSetDevice(e->cfg.device));
  const size_t S = (size_t)e->cfg.num_sessions, cells = 2 * (size_t)kDcTable * S;
  std::vector<int32_t> frames, counts;
  std::vector<uint16_t> cks;
  hipError_t rc = hipSuccess;
  auto keep = [&](hipError_t r) {
    if (rc == hipSuccess) rc = r;
  };
  auto rd = [&](int32_t* dst, int f) { keep(read_field(dst, e->dcmp_st, f, S, e->stream)); };
  rd(status, kDcStatus);
  rd(n_events, kDcEvents);
  rd(first_call, kDcFirstCall);
  rd(first_frame, kDcFirstFrame);
  rd(first_local, kDcFirstLocal);
  rd(first_remote, kDcFirstRemote);
  rd(refused, kDcRefused);
  if (history || pending) {
    frames.resize(cells);
    cks.resize(cells);
    counts.resize(2 * S);  // (kDcHist and kDcPend are neighbours)
    static_assert(kDcPend == kDcHist + 1, "the two counts are read in one copy");
    keep(hipMemcpyAsync(frames.data(), e->dcmp_frames, 4 * cells, hipMemcpyDeviceToHost, e->stream));
    keep(hipMemcpyAsync(cks.data(), e->dcmp_cks, 2 * cells, hipMemcpyDeviceToHost, e->stream));
    keep(hipMemcpyAsync(counts.data(), e->dcmp_st + (size_t)kDcHist * S, 4 * 2 * S, hipMemcpyDeviceToHost, e->stream));
  }
  const hipError_t waited = hipStreamSynchronize(e->stream);  // (before the vectors can be freed)
  HIP_TRY(rc);
  HIP_TRY(waited);
  // a table as [2][32][S]: the frames (-1 past the session's entries), then the checksums (0)
  int32_t* outs[2] = {history, pending};
  for (int T = 0; T < 2; T++) {
    if (!outs[T]) continue;
    for (size_t i = 0; i < (size_t)kDcTable; i++)
      for (size_t s = 0; s < S; s++) {
        const bool held = (int32_t)i < counts[(size_t)T * S + s];
        const size_t src = ((size_t)T * kDcTable + i) * S + s;
        outs[T][i * S + s] = held ? frames[src] : kNull;
        outs[T][((size_t)kDcTable + i) * S + s] = held ? (int32_t)cks[src] : 0;
      }
  }
  return GGRS_OK;
}

}  // extern "C"
