// spectator.hip -- batched SpectatorSession: S spectators, each following one host's confirmed
// input stream over its own network, one lane per session.
//
// Replaces (caspark/ggrs 0.10.2):
//   SpectatorSession::advance_frame   src/sessions/p2p_spectator_session.rs:103-129
//   SpectatorSession::inputs_at_frame :168-197 (PredictionThreshold, SpectatorTooFarBehind, the
//                                     Disconnected status of a player the host reported gone)
//   handle_event Event::Input         :218-231 (last_recv_frame, host_connect_status copied from the
//                                     host endpoint only when an input arrives)
//   UdpProtocol::on_input             src/network/protocol.rs:575-585 (peer_connect_status: sticky
//                                     disconnected, maximum last_frame, on every message)
//   + the ex_game handler's AdvanceFrame (examples/ex_game/ex_game.rs:115-127).
//
// One call c of one session:
//   1. the frames (last_recv, recv_upto[c]] arrive; the call's connect-status note is merged into
//      the endpoint's status (pending), which the session copies when at least one frame arrived;
//   2. n = last_recv - current_frame > max_frames_behind ? catchup_speed : 1;
//   3. n x { f = current_frame + 1; last_recv < f: PredictionThreshold; last_recv >= f + 60
//      (SPECTATOR_BUFFER_SIZE: slot f % 60 already holds a newer frame): SpectatorTooFarBehind;
//      else AdvanceFrame with row f, player k Disconnected iff disconnected[k] && last_frame[k] < f }.
// The reference returns the error of iteration i with `?`, dropping the i requests it had built
// while keeping current_frame advanced.  With catchup_speed == 1 or catchup_speed <
// max_frames_behind < 60 (the builder's rule, builder.rs:214-248, and this ABI's) that is never
// observable: n > 1 only when last_recv - current_frame > max_frames_behind > n, so all n frames
// have arrived, and last_recv < f + 60 at the first iteration holds at the later ones.  Both exits
// can only hit the first iteration, and the kernel decides a call's advance count there.
//
// Kernel shape: a session's BoxState and its integers (current_frame, last_recv, the effective and
// pending connect status, counters) stay in registers for the launch's n_calls calls.  Each lane
// walks its own calls.  One loop iteration = for the lanes between calls, the next call's integer
// work (its arrival word and note word, the advance count); then one AdvanceFrame for every lane
// that has one left, each at its own frame.  A lane spends max(1, advanced) iterations on a call,
// so a wave's cost is its slowest session's total over the launch, not the sum over calls of the
// slowest session of each call.  (Letting a lane run through its waiting calls in an inner loop
// was 2.3 times slower at catchup_speed 3: with 64 differently stalled lanes some lane is nearly
// always in such a run, and every pass of the inner loop is paid by the whole wave.)  The input row of frame f lives at rows[f % cap][s] whatever call
// advances it, so the next frame's dword is loaded one iteration ahead of its use (one wave per
// SIMD at 65,536 sessions: nothing else hides a load).  Arrival rows are stored four calls to a
// 16-byte group per session ([cap/4][S][4]): a lane loads its next group while it works through
// the current one, so a run of waiting calls -- integer work only, no step to hide a load behind --
// pays one exposed load per four calls instead of one per call.
#include <algorithm>
#include <string>
#include <vector>

#include "common.h"
#include "spectator_engine.h"

using namespace ggrs;

namespace {

constexpr int kSpecBlock = 64;     // one wave per block: waves spread over every SIMD of every CU
constexpr int kSpecBuffer = 60;    // SPECTATOR_BUFFER_SIZE (p2p_spectator_session.rs:17)
constexpr int32_t kNullFrame = GGRS_NULL_FRAME;

// per-session integers, [spec_fields(P)][S]
enum : int { kCur = 0, kLastRecv, kWaited, kErr, kDisc, kLast0 };
// kDisc: bits 0..3 the session's host_connect_status[k].disconnected, bits 4..7 the endpoint's
// (pending); kLast0 + k: the session's last_frame[k]; kLast0 + P + k: the endpoint's
constexpr int spec_fields(int p) { return kLast0 + 2 * p; }

struct SpecParams {
  int64_t S;
  int32_t cap;        // input rows held
  int32_t acap;       // arrival rows held (a multiple of 4)
  int32_t c0, n;      // calls c0 .. c0 + n - 1
  union {
    struct {
      int32_t row_lo, row_hi;  // input rows [row_lo, row_hi) are held when the launch starts
    };
    // the kFeed form, in their place (the table-fed kernels' arguments stay as they were): [S],
    // session s holds the rows (feed_last[s] - cap, feed_last[s]]
    const int32_t* feed_last;
  };
  int32_t mfb, speed;
  int32_t trace_cap;
  uint32_t* cur;      // [F][S]
  int32_t* sst;       // [spec_fields(P)][S]
  const uint32_t* rows;   // [cap][S] one padded dword per (frame, session), row f % cap
  const int4* recv;   // [acap / 4][S] recv_upto of calls 4 g .. 4 g + 3, group (c % acap) / 4
  const int4* notes;  // [acap / 4][S] GGRS_SPECTATOR_NOTE or 0, the same layout
  uint8_t* adv;       // [trace_cap][S]
  uint16_t* ck;       // [trace_cap][S]
};

__global__ void spec_init_kernel(int32_t* sst, int64_t S, int32_t fields) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)fields * S) return;
  const int f = (int)(i / S);
  sst[i] = (f == kWaited || f == kErr || f == kDisc) ? 0 : kNullFrame;
}

// [n][S][P] input bytes -> one dword per (frame, session) at row (f0 + k) % cap
__global__ void spec_pack_kernel(const uint8_t* src, uint32_t* rows, int64_t S, int32_t P, int32_t n, int32_t f0,
                                 int32_t cap) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)n * S) return;
  const int64_t k = i / S, s = i % S;
  uint32_t w = 0;
  for (int j = 0; j < P; j++) w |= (uint32_t)src[i * P + j] << (8 * j);
  rows[(((int64_t)f0 + k) % cap) * S + s] = w;
}

// [n][S] arrival words of calls c0 .. c0 + n - 1 -> the grouped table ([acap / 4][S][4]); src null: zeros
__global__ void spec_arrivals_kernel(const int32_t* src, int32_t* dst, int64_t S, int32_t n, int32_t c0, int32_t acap) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)n * S) return;
  const int64_t k = i / S, s = i % S;
  const int64_t slot = ((int64_t)c0 + k) % acap;
  dst[((slot / 4) * S + s) * 4 + (slot & 3)] = src ? src[i] : 0;
}

// kFeed: the packet-fed engine (spectator_ingest.hip).  Each session follows a host on its own clock,
// so the window of held rows is per session.  The feed delivers a session's frames consecutively, so
// slot f % cap of session s holds frame f exactly when L - cap < f <= L, L the feed's last_recv of the
// session when the launch starts: one [S] word instead of the lane-uniform (row_lo, row_hi), no tags.
// A call's arrival word is the feed's last_recv at that call (<= L, so the not-yet-added stop cannot
// happen) or kSpecFeedStop, at the call whose packet stopped the session.
template <int P, bool kTrace, bool kFeed>
__global__ __launch_bounds__(kSpecBlock) void spectator_kernel(SpecParams p) {
  const int64_t s = (int64_t)blockIdx.x * kSpecBlock + threadIdx.x;
  if (s >= p.S) return;
  const int64_t S = p.S;
  int32_t feed_hi = 0;
  if constexpr (kFeed) feed_hi = p.feed_last[s] + 1;
  // the session holds the rows [row_lo(), row_hi()) when the launch starts (kFeed: row_lo() may be
  // below 0, no frame is)
  auto row_lo = [&]() -> int32_t {
    if constexpr (kFeed) return feed_hi - p.cap;
    else return p.row_lo;
  };
  auto row_hi = [&]() -> int32_t {
    if constexpr (kFeed) return feed_hi;
    else return p.row_hi;
  };
  BoxState<P> st;
  load_state<P>(st, p.cur + s, S);
  int32_t* const sst = p.sst + s;
  int32_t cur = sst[(int64_t)kCur * S], lrecv = sst[(int64_t)kLastRecv * S];
  int32_t waited = sst[(int64_t)kWaited * S], err = sst[(int64_t)kErr * S];
  uint32_t disc = (uint32_t)sst[(int64_t)kDisc * S];
  int32_t el[P], pl[P];
#pragma unroll
  for (int k = 0; k < P; k++) {
    el[k] = sst[(int64_t)(kLast0 + k) * S];
    pl[k] = sst[(int64_t)(kLast0 + P + k) * S];
  }
  uint16_t ck = 0;
  if constexpr (kTrace) ck = fletcher16_state<P>(st);

  // the dword of frame g, if the launch holds it (a frame outside the window is never advanced:
  // its session stops first)
  auto row_of = [&](int32_t g) -> uint32_t {
    return (g >= row_lo() && g < row_hi()) ? p.rows[(int64_t)(g % p.cap) * S + s] : 0u;
  };
  uint32_t in_next = row_of(cur + 1);
  int32_t c = 0, todo = 0, adv_n = 0;
  // the arrival group of the current call and the one after it
  const int32_t groups = p.acap / 4, g_last = (p.c0 + p.n - 1) / 4;
  auto group_at = [&](int32_t g) -> int64_t { return (int64_t)(g % groups) * S + s; };
  auto pick = [](const int4& v, int32_t j) -> int32_t { return j == 0 ? v.x : (j == 1 ? v.y : (j == 2 ? v.z : v.w)); };
  int32_t g_cur = p.c0 / 4;
  int4 rg = p.recv[group_at(g_cur)], ng = p.notes[group_at(g_cur)];
  int4 rg_n = rg, ng_n = ng;
  if (g_cur < g_last) {
    rg_n = p.recv[group_at(g_cur + 1)];
    ng_n = p.notes[group_at(g_cur + 1)];
  }
  for (;;) {
    // ---- the lane's next call, integer work only (one call per iteration: a lane working through a
    // run of waiting calls costs the wave nothing beyond the control pass every iteration has anyway)
    if (todo == 0) {
      if (c >= p.n) break;
      const int32_t call = p.c0 + c;
      const int32_t r = pick(rg, call & 3), note = pick(ng, call & 3);
      c++;
      if ((call & 3) == 3) {  // on to the next group; load the one after it
        rg = rg_n;
        ng = ng_n;
        g_cur++;
        if (g_cur < g_last) {
          rg_n = p.recv[group_at(g_cur + 1)];
          ng_n = p.notes[group_at(g_cur + 1)];
        }
      }
      if (err != GGRS_E_INVALID && err != GGRS_E_PRECONDITION) {
        if (kFeed && r == kSpecFeedStop) {
          err = GGRS_E_PRECONDITION;  // the feed stopped the session at this call (the reference's assert!)
        } else if (r > lrecv && r >= row_hi()) {
          err = GGRS_E_INVALID;  // a frame the host has not produced yet
        } else {
          // protocol.rs:575-585: the endpoint's status, on every message
          if (note & 1) {
            const int k = (note >> 1) & 3;
            const int32_t fr = (note >> 3) - 1;
            disc |= 16u << k;
#pragma unroll
            for (int j = 0; j < P; j++)
              if (j == k) pl[j] = max(pl[j], fr);
          }
          // :218-231: Event::Input
          if (r > lrecv) {
            lrecv = r;
            disc = (disc & 0xf0u) | (disc >> 4);
#pragma unroll
            for (int j = 0; j < P; j++) el[j] = pl[j];
          }
          const int32_t f = cur + 1;
          if (lrecv < f) {
            waited++;  // PredictionThreshold
          } else if (lrecv >= f + kSpecBuffer) {
            err = GGRS_E_TOO_FAR_BEHIND;  // stays: current_frame no longer moves, last_recv only grows
          } else if (f < row_lo()) {
            err = GGRS_E_PRECONDITION;  // the row left the engine's window
          } else {
            todo = (lrecv - cur > p.mfb) ? p.speed : 1;
            adv_n = todo;
          }
        }
      }
      if constexpr (kTrace) {
        if (todo == 0) {
          const int64_t t = (int64_t)(call % p.trace_cap) * S + s;
          p.adv[t] = 0;
          p.ck[t] = ck;
        }
      }
    }
    // ---- one AdvanceFrame of every lane that has one
    if (todo > 0) {
      const int32_t f = cur + 1;
      uint32_t dmask = 0;
#pragma unroll
      for (int k = 0; k < P; k++) dmask |= (((disc >> k) & 1u) != 0 && el[k] < f) ? (1u << k) : 0u;
      advance_state<P>(st, in_next, dmask);
      cur = f;
      todo--;
      in_next = row_of(cur + 1);
      if constexpr (kTrace) {
        if (todo == 0) {
          ck = fletcher16_state<P>(st);
          const int64_t t = (int64_t)((p.c0 + c - 1) % p.trace_cap) * S + s;
          p.adv[t] = (uint8_t)adv_n;
          p.ck[t] = ck;
        }
      }
    }
  }
  store_state<P>(st, p.cur + s, S);
  sst[(int64_t)kCur * S] = cur;
  sst[(int64_t)kLastRecv * S] = lrecv;
  sst[(int64_t)kWaited * S] = waited;
  sst[(int64_t)kErr * S] = err;
  sst[(int64_t)kDisc * S] = (int32_t)disc;
#pragma unroll
  for (int k = 0; k < P; k++) {
    sst[(int64_t)(kLast0 + k) * S] = el[k];
    sst[(int64_t)(kLast0 + P + k) * S] = pl[k];
  }
}

}  // namespace

extern "C" {

int ggrs_spectator_engine_destroy(ggrs_spectator_engine_t* e) {
  if (!e) return GGRS_OK;
  (void)hipSetDevice(e->cfg.device);
  if (e->stream) (void)hipStreamSynchronize(e->stream);
  void* bufs[] = {e->cur, e->sst, e->rows, e->recv, e->notes, e->adv, e->ck, e->staging};
  for (void* b : bufs)
    if (b) (void)hipFree(b);
  spectator_ingest_free(e);
  spectator_poll_free(e);
  spectator_events_free(e);
  e->timer.destroy();
  if (e->stream) (void)hipStreamDestroy(e->stream);
  delete e;
  return GGRS_OK;
}

// SessionBuilder::start_spectator_session (builder.rs:310-338) with with_max_frames_behind /
// with_catchup_speed's checks (:214-248) + SpectatorSession::new (p2p_spectator_session.rs:43-71)
// + State::new (ex_game.rs:246-269)
int ggrs_spectator_engine_create(const ggrs_spectator_config_t* cfg, ggrs_spectator_engine_t** out) {
  if (!cfg || !out) return set_error(GGRS_E_INVALID, "null argument");
  *out = nullptr;
  ggrs_spectator_config_t c = *cfg;
  if (c.num_sessions < 1) return set_error(GGRS_E_INVALID, "num_sessions must be >= 1");
  if (c.num_players < 1 || c.num_players > 4) return set_error(GGRS_E_INVALID, "num_players must be in 1..4 (ex_game.rs:70)");
  if (c.max_frames_behind < 1) return set_error(GGRS_E_INVALID, "Max frames behind cannot be smaller than 1.");
  if (c.max_frames_behind >= kSpecBuffer)
    return set_error(GGRS_E_INVALID, "Max frames behind cannot be larger or equal than the Spectator buffer size (60)");
  if (c.catchup_speed < 1) return set_error(GGRS_E_INVALID, "Catchup speed cannot be smaller than 1.");
  if (c.catchup_speed != 1 && c.catchup_speed >= c.max_frames_behind)
    return set_error(GGRS_E_INVALID, "Catchup speed cannot be larger or equal than the allowed maximum frames behind host");
  if (c.input_capacity == 0) c.input_capacity = 256;
  if (c.input_capacity < kSpecBuffer + 4)
    return set_error(GGRS_E_INVALID, "input_capacity must be >= %d (the spectator buffer and a margin)", kSpecBuffer + 4);
  if (c.trace_capacity < 0) return set_error(GGRS_E_INVALID, "trace_capacity must be >= 0");
  ggrs_spectator_engine* e = new ggrs_spectator_engine();
  e->cfg = c;
  e->F = state_fields(c.num_players);
  e->cap = c.input_capacity;
  e->acap = (c.input_capacity + 3) / 4 * 4;
  auto fail = [&](int rc) {
    std::string msg = ggrs_last_error();
    ggrs_spectator_engine_destroy(e);
    set_error(rc, "%s", msg.c_str());
    return rc;
  };
#define CTRY(expr)                                                                      \
  do {                                                                                  \
    hipError_t e_ = (expr);                                                             \
    if (e_ != hipSuccess) return fail(set_error(GGRS_E_HIP, "%s: %s", #expr, hipGetErrorString(e_))); \
  } while (0)
  const int64_t S = c.num_sessions;
  const int P = c.num_players;
  const int fields = spec_fields(P);
  CTRY(hipSetDevice(c.device));
  CTRY(hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking));
  if (e->timer.create()) return fail(GGRS_E_HIP);
  CTRY(hipMalloc(&e->cur, sizeof(uint32_t) * e->F * S));
  CTRY(hipMalloc(&e->sst, sizeof(int32_t) * fields * S));
  CTRY(hipMalloc(&e->rows, sizeof(uint32_t) * (size_t)e->cap * S));
  CTRY(hipMalloc(&e->recv, sizeof(int32_t) * (size_t)e->acap * S));
  CTRY(hipMalloc(&e->notes, sizeof(int32_t) * (size_t)e->acap * S));
  CTRY(hipMemsetAsync(e->rows, 0, sizeof(uint32_t) * (size_t)e->cap * S, e->stream));
  CTRY(hipMemsetAsync(e->recv, 0xff, sizeof(int32_t) * (size_t)e->acap * S, e->stream));
  CTRY(hipMemsetAsync(e->notes, 0, sizeof(int32_t) * (size_t)e->acap * S, e->stream));
  if (c.trace_capacity > 0) {
    CTRY(hipMalloc(&e->adv, (size_t)c.trace_capacity * S));
    CTRY(hipMalloc(&e->ck, sizeof(uint16_t) * (size_t)c.trace_capacity * S));
    CTRY(hipMemsetAsync(e->adv, 0, (size_t)c.trace_capacity * S, e->stream));
    CTRY(hipMemsetAsync(e->ck, 0, sizeof(uint16_t) * (size_t)c.trace_capacity * S, e->stream));
  }
  spec_init_kernel<<<grid_of((int64_t)fields * S, 256), 256, 0, e->stream>>>(e->sst, S, fields);
  dispatch_players(P, [&](auto PC) {
    constexpr int PP = decltype(PC)::value;
    init_states_kernel<PP><<<grid_of(S, 256), 256, 0, e->stream>>>(e->cur, S);
  });
  CTRY(hipGetLastError());
  CTRY(hipStreamSynchronize(e->stream));
#undef CTRY
  *out = e;
  return GGRS_OK;
}

int ggrs_spectator_engine_config(const ggrs_spectator_engine_t* e, ggrs_spectator_config_t* out) {
  if (!e || !out) return set_error(GGRS_E_INVALID, "null argument");
  *out = e->cfg;
  return GGRS_OK;
}

int ggrs_spectator_add_inputs(ggrs_spectator_engine_t* e, int32_t first_frame, int32_t n, const uint8_t* inputs) {
  if (!e || (!inputs && n > 0)) return set_error(GGRS_E_INVALID, "null argument");
  if (e->pkt) return set_error(GGRS_E_STATE, "a packet-fed engine takes its inputs from ggrs_spectator_receive_packets");
  if (n < 0) return set_error(GGRS_E_INVALID, "n_frames must be >= 0");
  if (first_frame != e->next_input_frame)
    return set_error(GGRS_E_INVALID, "inputs must be added sequentially (expected frame %d, got %d)",
                     e->next_input_frame, first_frame);
  if (n == 0) return GGRS_OK;
  HIP_TRY(hipSetDevice(e->cfg.device));
  const int64_t S = e->cfg.num_sessions;
  const int P = e->cfg.num_players;
  // the newest input_capacity rows are kept: of a longer run only its tail is stored
  const int32_t skip = std::max(0, n - e->cap);
  const int32_t m = n - skip;
  const size_t bytes = (size_t)m * S * P;
  if (bytes > e->staging_bytes) {
    if (e->staging) HIP_TRY(hipFree(e->staging));
    e->staging = nullptr;
    e->staging_bytes = 0;
    HIP_TRY(hipMalloc(&e->staging, bytes));
    e->staging_bytes = bytes;
  }
  HIP_TRY(hipMemcpyAsync(e->staging, inputs + (size_t)skip * S * P, bytes, hipMemcpyHostToDevice, e->stream));
  spec_pack_kernel<<<grid_of((int64_t)m * S, 256), 256, 0, e->stream>>>(e->staging, e->rows, S, P, m, first_frame + skip,
                                                                       e->cap);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(e->stream));
  e->next_input_frame = first_frame + n;
  return GGRS_OK;
}

int ggrs_spectator_add_arrivals(ggrs_spectator_engine_t* e, int32_t first_call, int32_t n, const int32_t* recv_upto,
                                const int32_t* notes) {
  if (!e || (!recv_upto && n > 0)) return set_error(GGRS_E_INVALID, "null argument");
  if (e->pkt) return set_error(GGRS_E_STATE, "a packet-fed engine takes its arrivals from ggrs_spectator_receive_packets");
  if (n < 0) return set_error(GGRS_E_INVALID, "n_calls must be >= 0");
  if (first_call != e->next_arrival_call)
    return set_error(GGRS_E_INVALID, "arrivals must be added in call order (expected call %d, got %d)",
                     e->next_arrival_call, first_call);
  if (n == 0) return GGRS_OK;
  if ((int64_t)first_call + n - 1 - e->calls >= e->cap)
    return set_error(GGRS_E_INVALID, "arrival queue full (capacity %d calls)", e->cap);
  const int64_t S = e->cfg.num_sessions;
  if (notes) {
    const int P = e->cfg.num_players;
    for (int64_t i = 0; i < (int64_t)n * S; i++) {
      const int32_t v = notes[i];
      if (v == 0) continue;
      if (!(v & 1) || v < 0 || ((v >> 1) & 3) >= P)
        return set_error(GGRS_E_INVALID, "bad connect-status note %d (call %d, session %lld): GGRS_SPECTATOR_NOTE(player, "
                         "frame) of one of the session's players, frame >= -1", v, first_call + (int32_t)(i / S),
                         (long long)(i % S));
    }
  }
  HIP_TRY(hipSetDevice(e->cfg.device));
  // staged, then scattered into the grouped tables (four calls to a 16-byte group per session)
  const size_t words = (size_t)n * S, bytes = words * sizeof(int32_t) * 2;
  if (bytes > e->staging_bytes) {
    if (e->staging) HIP_TRY(hipFree(e->staging));
    e->staging = nullptr;
    e->staging_bytes = 0;
    HIP_TRY(hipMalloc(&e->staging, bytes));
    e->staging_bytes = bytes;
  }
  int32_t* st_recv = reinterpret_cast<int32_t*>(e->staging);
  int32_t* st_notes = st_recv + words;
  HIP_TRY(hipMemcpyAsync(st_recv, recv_upto, words * sizeof(int32_t), hipMemcpyHostToDevice, e->stream));
  if (notes) HIP_TRY(hipMemcpyAsync(st_notes, notes, words * sizeof(int32_t), hipMemcpyHostToDevice, e->stream));
  const unsigned grid = (unsigned)grid_of((int64_t)words, 256);
  spec_arrivals_kernel<<<grid, 256, 0, e->stream>>>(st_recv, reinterpret_cast<int32_t*>(e->recv), S, n, first_call,
                                                    e->acap);
  spec_arrivals_kernel<<<grid, 256, 0, e->stream>>>(notes ? st_notes : nullptr, reinterpret_cast<int32_t*>(e->notes), S, n,
                                                    first_call, e->acap);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(e->stream));
  e->next_arrival_call = first_call + n;
  return GGRS_OK;
}

int ggrs_spectator_advance_frames(ggrs_spectator_engine_t* e, int32_t n) {
  if (!e) return set_error(GGRS_E_INVALID, "null engine");
  if (n < 0) return set_error(GGRS_E_INVALID, "n_calls must be >= 0");
  if (n == 0) return GGRS_OK;
  if ((int64_t)e->calls + n > e->next_arrival_call)
    return set_error(GGRS_E_INVALID, "Missing arrivals: arrival rows are queued up to call %d, calls need up to %d",
                     e->next_arrival_call - 1, e->calls + n - 1);
  HIP_TRY(hipSetDevice(e->cfg.device));
  SpecParams p;
  p.S = e->cfg.num_sessions;
  p.cap = e->cap;
  p.acap = e->acap;
  p.c0 = e->calls;
  p.n = n;
  if (e->pkt) {
    p.feed_last = e->feed.last;
  } else {
    p.row_lo = std::max(0, e->next_input_frame - e->cap);
    p.row_hi = e->next_input_frame;
  }
  p.mfb = e->cfg.max_frames_behind;
  p.speed = e->cfg.catchup_speed;
  p.trace_cap = e->adv ? e->cfg.trace_capacity : 0;
  p.cur = e->cur;
  p.sst = e->sst;
  p.rows = e->rows;
  p.recv = e->recv;
  p.notes = e->notes;
  p.adv = e->adv;
  p.ck = e->ck;
  if (int rc = e->timer.before(e->stream)) return rc;
  const unsigned grid = (unsigned)grid_of(p.S, kSpecBlock);
  dispatch_players(e->cfg.num_players, [&](auto PC) {
    constexpr int PP = decltype(PC)::value;
    if (e->pkt) {
      if (p.trace_cap > 0) spectator_kernel<PP, true, true><<<grid, kSpecBlock, 0, e->stream>>>(p);
      else spectator_kernel<PP, false, true><<<grid, kSpecBlock, 0, e->stream>>>(p);
    } else {
      if (p.trace_cap > 0) spectator_kernel<PP, true, false><<<grid, kSpecBlock, 0, e->stream>>>(p);
      else spectator_kernel<PP, false, false><<<grid, kSpecBlock, 0, e->stream>>>(p);
    }
  });
  HIP_TRY(hipGetLastError());
  e->timer.count();
  e->calls += n;
  return GGRS_OK;
}

int ggrs_spectator_calls(const ggrs_spectator_engine_t* e, int32_t* out) {
  if (!e || !out) return set_error(GGRS_E_INVALID, "null argument");
  *out = e->calls;
  return GGRS_OK;
}

int ggrs_spectator_synchronize(ggrs_spectator_engine_t* e) {
  if (!e) return set_error(GGRS_E_INVALID, "null engine");
  HIP_TRY(hipSetDevice(e->cfg.device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return GGRS_OK;
}

int ggrs_spectator_read_sessions(ggrs_spectator_engine_t* e, int32_t* current_frame, int32_t* last_recv, int32_t* waited,
                                 int32_t* errors) {
  if (!e) return set_error(GGRS_E_INVALID, "null engine");
  HIP_TRY(hipSetDevice(e->cfg.device));
  const int64_t S = e->cfg.num_sessions;
  int32_t* dst[] = {current_frame, last_recv, waited, errors};
  const int fld[] = {kCur, kLastRecv, kWaited, kErr};
  for (int i = 0; i < 4; i++)
    if (dst[i]) HIP_TRY(hipMemcpyAsync(dst[i], e->sst + (int64_t)fld[i] * S, 4 * S, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return GGRS_OK;
}

int ggrs_spectator_read_state(ggrs_spectator_engine_t* e, int32_t session, uint8_t* out) {
  if (!e || !out) return set_error(GGRS_E_INVALID, "null argument");
  if (session < 0 || session >= e->cfg.num_sessions) return set_error(GGRS_E_INVALID, "session out of range");
  HIP_TRY(hipSetDevice(e->cfg.device));
  std::vector<uint32_t> w(e->F);
  for (int k = 0; k < e->F; k++)
    HIP_TRY(hipMemcpyAsync(&w[k], e->cur + (int64_t)k * e->cfg.num_sessions + session, 4, hipMemcpyDeviceToHost,
                           e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  serialize_state_bytes(w.data(), e->cfg.num_players, out);
  return GGRS_OK;
}

int ggrs_spectator_read_states(ggrs_spectator_engine_t* e, uint8_t* out) {
  if (!e || !out) return set_error(GGRS_E_INVALID, "null argument");
  HIP_TRY(hipSetDevice(e->cfg.device));
  const int64_t S = e->cfg.num_sessions;
  const size_t sb = 36 + 20 * (size_t)e->cfg.num_players;
  std::vector<uint32_t> soa((size_t)e->F * S);
  HIP_TRY(hipMemcpyAsync(soa.data(), e->cur, soa.size() * 4, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  std::vector<uint32_t> w(e->F);
  for (int64_t s = 0; s < S; s++) {
    for (int k = 0; k < e->F; k++) w[k] = soa[(size_t)k * S + s];
    serialize_state_bytes(w.data(), e->cfg.num_players, out + (size_t)s * sb);
  }
  return GGRS_OK;
}

int ggrs_spectator_read_trace(ggrs_spectator_engine_t* e, int32_t first_call, int32_t n, uint8_t* advanced,
                              uint16_t* checksums) {
  if (!e) return set_error(GGRS_E_INVALID, "null engine");
  if (!e->adv) return set_error(GGRS_E_PRECONDITION, "engine created with trace_capacity 0");
  const int32_t T = e->cfg.trace_capacity;
  if (n < 0 || first_call < 0 || (int64_t)first_call + n > e->calls || (int64_t)first_call + T < e->calls)
    return set_error(GGRS_E_INVALID, "trace calls out of the retained range");
  HIP_TRY(hipSetDevice(e->cfg.device));
  const int64_t S = e->cfg.num_sessions;
  for (int32_t i = 0; i < n; i++) {
    const int64_t row = (int64_t)((first_call + i) % T) * S;
    if (advanced) HIP_TRY(hipMemcpyAsync(advanced + (int64_t)i * S, e->adv + row, S, hipMemcpyDeviceToHost, e->stream));
    if (checksums)
      HIP_TRY(hipMemcpyAsync(checksums + (int64_t)i * S, e->ck + row, 2 * S, hipMemcpyDeviceToHost, e->stream));
  }
  HIP_TRY(hipStreamSynchronize(e->stream));
  return GGRS_OK;
}

int ggrs_spectator_timing_reset(ggrs_spectator_engine_t* e) {
  if (!e) return set_error(GGRS_E_INVALID, "null engine");
  HIP_TRY(hipSetDevice(e->cfg.device));
  return e->timer.reset(e->stream);
}

int ggrs_spectator_timing_stop(ggrs_spectator_engine_t* e) {
  if (!e) return set_error(GGRS_E_INVALID, "null engine");
  HIP_TRY(hipSetDevice(e->cfg.device));
  return e->timer.stop(e->stream);
}

int ggrs_spectator_timing_read(ggrs_spectator_engine_t* e, float* total_ms, int32_t* launches) {
  if (!e || !total_ms || !launches) return set_error(GGRS_E_INVALID, "null argument");
  HIP_TRY(hipSetDevice(e->cfg.device));
  return e->timer.read(e->stream, total_ms, launches);
}

}  // extern "C"
