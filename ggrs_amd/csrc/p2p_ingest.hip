// p2p_ingest.hip -- the packet feed of the any-network P2P engine (p2p_sched.hip): a session's remote
// inputs enter as the compressed Input messages its endpoint received, at the call that polled
// them, instead of as rows known in advance.  The receive side of the wire protocol,
// UdpProtocol::on_input, is ingest_device.h's (steps 1-4 and the kernel plan, shared with
// spectator_ingest.hip); here is what the P2P feed adds to it.  The packet's new frames are stored into
// the engine's own input rows -- the input ring doubles as the endpoint's recv_inputs -- and the
// call's arrival row (the table ggrs_p2p_add_arrivals takes from the host) is written on the device.
// The scheduled kernels read the same rows and tables as before.
//
// The P2P feed's own, by on_input's steps as ingest_device.h numbers them:
//   -  a packet input is the remote players' bytes in ascending player order; they are gathered from
//      and scattered to the columns of a row word.
//   2. a kept reference frame whose row slot holds another frame (row_tag) stops the session with
//      GGRS_E_PRECONDITION, the engine's rule for a remote input no longer in the rows.
//   4. so does a frame to deliver whose row slot holds another frame; a last frame beyond the call
//      stops the session with GGRS_E_INVALID (the arrival table's rule) before anything is stored.
//   5. arrive[c] = last_recv, events[c] = the caller's.
// How a stop reaches the session: the scheduled kernels stop a session at the call whose arrival
// names a frame after it (GGRS_E_INVALID), so a stopping call's arrival row holds such a frame (the
// packet's last frame for 4's second case, c + 1 otherwise) and the feed's stop word remembers the
// call; after the launch that ran it, ingest_stops_kernel turns that session's error into
// GGRS_E_PRECONDITION.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "common.h"
#include "ingest_device.h"
#include "p2p_engine.h"

using namespace ggrs;

namespace {

constexpr int kIngestTags = 2048;        // row tags kept in LDS up to this input_capacity
constexpr int32_t kStoppedInvalid = -2;  // the stop word: <= this, stopped with GGRS_E_INVALID at call -2 - v

struct IngestParams {
  IngestFeed feed;
  int32_t tags_lds;        // the row tags are copied to LDS (cap <= kIngestTags and room for them)
  int32_t Pp;              // row word bytes
  uint32_t rpos;           // byte j: the column (player) of remote player j in a row word
  uint8_t* inputs;         // [cap][S] row words
  const int32_t* row_tag;  // [cap]
  int32_t* arrive;         // [cap][S]
  uint8_t* events;         // [cap][S]
  const uint8_t* ev_in;    // [n][S] or null
  uint32_t ev_mask;        // (1 << num_players) - 1: the bits of ev_in that name a player
};

// The P2P feed's rows (ingest_device.h's row policy), for one thread's session s.  kB: the remote
// players; l_tags: the row tags in LDS when they fit (tags_lds) -- a session reads several per call,
// each a memory latency on its chain of calls otherwise.
template <int kB>
struct P2PRows {
  const IngestParams& p;
  const int64_t s;
  const int32_t* const l_tags;

  __device__ inline int32_t tag_at(int32_t slot) const { return p.tags_lds ? l_tags[slot] : p.row_tag[slot]; }
  // the remote players' bytes of a row word, packed in ascending player order (InputBytes::
  // to_player_inputs over the endpoint's handles, protocol.rs:622), and back
  __device__ inline uint32_t load_reference(int32_t rslot, int32_t rf, bool& held) const {
    const uint8_t* w = p.inputs + ((int64_t)rslot * p.feed.S + s) * p.Pp;
    uint32_t v = 0;
    for (int j = 0; j < kB; j++) v |= (uint32_t)w[(p.rpos >> (8 * j)) & 0xffu] << (8 * j);
    held = tag_at(rslot) == rf;
    return v;
  }
  __device__ inline void store(int32_t slot, uint32_t v) const {
    const int32_t Pp = p.Pp;
    uint8_t* w = p.inputs + ((int64_t)slot * p.feed.S + s) * Pp;
    if (kB == Pp) {  // every player remote: the whole word
      if (Pp == 1) *w = (uint8_t)v;
      else if (Pp == 2) *reinterpret_cast<uint16_t*>(w) = (uint16_t)v;
      else *reinterpret_cast<uint32_t*>(w) = v;
    } else {
      for (int j = 0; j < kB; j++) w[(p.rpos >> (8 * j)) & 0xffu] = (uint8_t)(v >> (8 * j));
    }
  }
  __device__ inline IngestDelivery check_delivery(int32_t start, int32_t s_slot, int32_t last, int32_t lastf,
                                                  int32_t c) const {
    if (lastf > c) return IngestDelivery::kStopBeyondCall;  // a frame the peer cannot have sent yet
    bool held = true;
    for (int32_t f = start, slot = s_slot; f <= lastf; ++f, slot = slot + 1 == p.feed.cap ? 0 : slot + 1)
      if (f > last) held &= tag_at(slot) == f;
    return held ? IngestDelivery::kDeliver : IngestDelivery::kStop;
  }
  __device__ inline void begin_call(int32_t) const {}  // (the call's events are read with its outputs)
  __device__ inline void write_outputs(int32_t k, int32_t c, int64_t o, const IngestOutcome& r, int32_t last,
                                       int32_t& stop) const {
    if (r.stopped) stop = r.marker ? kStoppedInvalid - c : c;
    p.arrive[o] = r.stopped ? (r.marker ? r.marker : c + 1) : last;
    // (bits at or above num_players name no player and are dropped here: bit 4 of a stored
    // byte is the scheduled kernels' own peer-report flag)
    p.events[o] = p.ev_in ? (uint8_t)(p.ev_in[(int64_t)k * p.feed.S + s] & p.ev_mask) : (uint8_t)0;
  }
};

template <int kB>
__global__ __launch_bounds__(kIngestBlock) void p2p_ingest_kernel(IngestParams p) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];  // (IngestLane), then [cap] the row tags (tags_lds)
  const IngestLane b(p.feed, smem);
  int32_t* const l_tags = reinterpret_cast<int32_t*>(b.l_own);
  if (p.tags_lds)  // (the first group's barrier orders the copy before its readers)
    for (int i = b.t; i < p.feed.cap; i += kIngestBlock) l_tags[i] = p.row_tag[i];
  P2PRows<kB> rows{p, b.s, l_tags};
  ingest_walk<kB>(p.feed, b, rows);
}

// After a launch of calls: the sessions the feed stopped at a call now run hold the arrival table's
// GGRS_E_INVALID; theirs is the reference's panic.
__global__ void ingest_stops_kernel(int32_t* err, const int32_t* stop, int64_t S, int32_t calls_run) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
  const int32_t st = stop[s];
  if (st >= 0 && st < calls_run && err[s] == GGRS_E_INVALID) err[s] = GGRS_E_PRECONDITION;
}

int remote_players(const ggrs_p2p_engine* e, uint32_t* rpos) {
  int B = 0;
  uint32_t r = 0;
  for (int k = 0; k < e->cfg.num_players; k++)
    if (!((e->cfg.local_mask >> k) & 1)) r |= (uint32_t)k << (8 * B++);
  if (rpos) *rpos = r;
  return B;
}

}  // namespace

namespace ggrs {

int p2p_ingest_free(ggrs_p2p_engine* e) {
  e->feed.release();
  return GGRS_OK;
}

int p2p_ingest_launch(ggrs_p2p_engine* e, int32_t first_call, int32_t n, const int32_t* start_frame,
                      const int32_t* packet_len, const uint8_t* packets, const uint8_t* events) {
  IngestParams p;
  size_t tag_bytes = e->cap <= kIngestTags ? sizeof(int32_t) * (size_t)e->cap : 0;
  if (ingest_call_bytes(e->feed.stride) + tag_bytes > kIngestLds) tag_bytes = 0;
  const IngestPlan plan = ingest_plan(e->feed.stride, n, tag_bytes);
  p.feed = ingest_feed(e->feed, e->cfg.num_sessions, e->cap, e->cfg.max_prediction, first_call, n, plan.G, start_frame,
                       packet_len, packets);
  p.tags_lds = tag_bytes != 0;
  const int B = remote_players(e, &p.rpos);
  p.Pp = e->Pp;
  p.inputs = e->inputs;
  p.row_tag = e->row_tag;
  p.arrive = e->arrive;
  p.events = e->events;
  p.ev_in = events;
  p.ev_mask = (1u << e->cfg.num_players) - 1u;
  if (int rc = e->timer.before(e->stream)) return rc;
  const int64_t grid = grid_of(p.feed.S, kIngestBlock);
  dispatch_players(B, [&](auto BC) {
    constexpr int BB = decltype(BC)::value;
    p2p_ingest_kernel<BB><<<grid, kIngestBlock, plan.lds, e->stream>>>(p);
  });
  HIP_TRY(hipGetLastError());
  e->timer.count();
  return GGRS_OK;
}

int p2p_ingest_after_advance(ggrs_p2p_engine* e) {
  const int64_t S = e->cfg.num_sessions;
  ingest_stops_kernel<<<grid_of(S, 256), 256, 0, e->stream>>>(p2p_sched_errors(e), e->feed.stop, S, e->current_frame);
  HIP_TRY(hipGetLastError());
  return GGRS_OK;
}

}  // namespace ggrs

extern "C" {

int ggrs_p2p_set_packet_feed(ggrs_p2p_engine_t* e, int32_t max_packet_inputs, int32_t packet_stride) {
  if (!e) return set_error(GGRS_E_INVALID, "null engine");
  if (e->current_frame != 0 || e->next_arrival_call != 0)
    return set_error(GGRS_E_STATE, "the packet feed is part of the session's configuration (set before the first call)");
  if (!e->sched) return set_error(GGRS_E_STATE, "the packet feed needs ggrs_p2p_set_arrival_schedule(e, 1)");
  const int B = remote_players(e, nullptr);
  if (B < 1) return set_error(GGRS_E_INVALID, "the packet feed needs a remote player");
  if (int rc = PacketFeedState::check(B, max_packet_inputs, packet_stride, kIngestMaxStride)) return rc;
  HIP_TRY(hipSetDevice(e->cfg.device));
  if (int rc = e->feed.reset((size_t)e->cfg.num_sessions, (size_t)e->cap, max_packet_inputs, packet_stride, e->stream))
    return rc;
  e->pkt = 1;
  return GGRS_OK;
}

int ggrs_p2p_receive_packets(ggrs_p2p_engine_t* e, int32_t first_call, int32_t n, const int32_t* start_frame,
                             const int32_t* packet_len, const uint8_t* packets, const uint8_t* events,
                             int32_t on_device) {
  if (!e) return set_error(GGRS_E_INVALID, "null engine");
  if (!e->sched || !e->pkt) return set_error(GGRS_E_STATE, "receiving packets needs ggrs_p2p_set_packet_feed");
  if (n < 0) return set_error(GGRS_E_INVALID, "n_calls must be >= 0");
  if (first_call != e->next_arrival_call)
    return set_error(GGRS_E_INVALID, "packets must be received in call order (expected call %d, got %d)",
                     e->next_arrival_call, first_call);
  if (n == 0) return GGRS_OK;
  if (!start_frame || !packet_len || !packets) return set_error(GGRS_E_INVALID, "null argument");
  if ((int64_t)first_call + n - 1 - e->current_frame >= e->cap)
    return set_error(GGRS_E_INVALID, "arrival queue full (capacity %d calls)", e->cap);
  if ((int64_t)first_call + n > e->next_input_frame)
    return set_error(GGRS_E_INVALID, "the input rows of calls up to %d must be added first (added up to %d)",
                     first_call + n - 1, e->next_input_frame - 1);
  if (on_device && ((uintptr_t)packets & 3))
    return set_error(GGRS_E_INVALID, "device packets must be dword aligned");
  HIP_TRY(hipSetDevice(e->cfg.device));
  const size_t S = (size_t)e->cfg.num_sessions;
  if (!on_device)  // through the feed's staging buffer, the calls' events beside them
    if (int rc = e->feed.stage((size_t)n * S, &start_frame, &packet_len, &packets, &events, e->stream)) return rc;
  if (e->peer_reports)  // (a slot's report from cap calls ago is not this call's)
    for (int32_t k = 0; k < n;) {
      const int32_t slot = (first_call + k) % e->cap;
      const int32_t m = std::min(n - k, e->cap - slot);
      HIP_TRY(hipMemsetAsync(e->peer_reports + (int64_t)slot * S, 0, sizeof(int32_t) * m * S, e->stream));
      k += m;
    }
  if (int rc = p2p_ingest_launch(e, first_call, n, start_frame, packet_len, packets, events)) return rc;
  // host sources: the caller may reuse its arrays on return (as ggrs_p2p_add_arrivals); device
  // sources are read in stream order, nothing to wait for
  if (!on_device) HIP_TRY(hipStreamSynchronize(e->stream));
  e->next_arrival_call = first_call + n;
  return GGRS_OK;
}

int ggrs_p2p_read_packet_results(ggrs_p2p_engine_t* e, int32_t first_call, int32_t n, int32_t* status,
                                 int32_t* ack_frame) {
  if (!e) return set_error(GGRS_E_INVALID, "null engine");
  if (!e->sched || !e->pkt) return set_error(GGRS_E_STATE, "packet results exist with ggrs_p2p_set_packet_feed only");
  HIP_TRY(hipSetDevice(e->cfg.device));
  return e->feed.read(first_call, n, e->next_arrival_call, e->cap, e->cfg.num_sessions, status, ack_frame, e->stream);
}

}  // extern "C"
