// spectator_ingest.hip -- the packet feed of the spectator engine (spectator.hip): a session's host
// inputs enter as the compressed Input messages its endpoint received, at the call that polled them,
// instead of as dense rows and a recv_upto table known in advance.  The receive side of the wire
// protocol, UdpProtocol::on_input, is ingest_device.h's (steps 1-4 and the kernel plan, shared with
// p2p_ingest.hip); here is what the spectator feed adds to it, up to SpectatorSession::handle_event's
// Event::Input (p2p_spectator_session.rs:218-231).  The packet's new frames are stored into the
// session's input rows -- the row ring doubles as the endpoint's recv_inputs -- and the call's
// arrival word (recv_upto) and note are written into the grouped tables spectator_kernel reads.  The
// feed is the only writer of a packet-fed engine's rows and tables.
//
// The spectator feed's own, by on_input's steps as ingest_device.h numbers them:
//   -  a packet input is all players' bytes, the whole padded dword of a row: the reference is one dword
//      load and delivery one dword store per frame.  Every lane is at its own frame and ring slot; with
//      hosts on different clocks the 64 row stores of a wave go to up to 64 different lines (rows is
//      [cap][S], laid out for spectator_kernel's coalesced reads).
//   4. the host runs on its own clock: no bound by the call.
//   5. recv_upto[c] = ack[c] = last_recv; the call's note goes into the note table whatever became of
//      the packet (:575-585 precedes the decode).
// A stopped session's arrival word is kSpecFeedStop from the stopping call on, which the kFeed form of
// spectator_kernel turns into GGRS_E_PRECONDITION at that call.
// Why no row tags: a session's delivery is consecutive and gap-free, so slot f % cap holds frame f
// exactly when last_recv - cap < f <= last_recv.  The reference frame start - 1 lies in
// [last_recv - 2 max_prediction, last_recv], inside that window because input_capacity >
// 2 max_prediction + max_packet_inputs (ggrs_spectator_set_packet_feed), and is read before the
// packet's own stores.
#include <hip/hip_runtime.h>

#include "common.h"
#include "ingest_device.h"
#include "spectator_engine.h"

using namespace ggrs;

namespace {

struct SpecIngestParams {
  IngestFeed feed;
  int32_t acap;
  uint32_t* rows;           // [cap][S] one padded dword per (frame, session)
  int32_t* recv;            // [acap / 4][S][4]
  int32_t* notes;           // [acap / 4][S][4]
  const int32_t* notes_in;  // [n][S] or null
};

// The spectator feed's rows (ingest_device.h's row policy), for one thread's session s (`live`: it has
// one).  kP: the players.
template <int kP>
struct SpecRows {
  const SpecIngestParams& p;
  const int64_t s;
  const bool live;
  int32_t ai;    // the call's slot in the arrival tables
  int32_t note;  // the call's note

  __device__ inline uint32_t load_reference(int32_t rslot, int32_t, bool&) const { return p.rows[(int64_t)rslot * p.feed.S + s]; }
  __device__ inline void store(int32_t slot, uint32_t v) const { p.rows[(int64_t)slot * p.feed.S + s] = v; }
  __device__ inline IngestDelivery check_delivery(int32_t, int32_t, int32_t, int32_t, int32_t) const {
    return IngestDelivery::kDeliver;
  }
  // the call's note: a malformed one counts as none (the host path refuses it before the launch).
  // Loaded ahead of the packet, so that its latency overlaps the reference row's.
  __device__ inline void begin_call(int32_t k) {
    note = (live && p.notes_in) ? p.notes_in[(int64_t)k * p.feed.S + s] : 0;
    if (!(note & 1) || note < 0 || ((note >> 1) & 3) >= kP) note = 0;
  }
  // the call's arrival and note words for spectator_kernel (ai steps with the calls of a thread that
  // has a session; no other thread uses it)
  __device__ inline void write_outputs(int32_t, int32_t c, int64_t, const IngestOutcome& r, int32_t last, int32_t& stop) {
    if (r.stopped) stop = c;
    const int64_t a = (((int64_t)(ai >> 2) * p.feed.S + s) << 2) + (ai & 3);
    p.recv[a] = stop != kNull ? kSpecFeedStop : last;
    p.notes[a] = note;
    ai = ai + 1 == p.acap ? 0 : ai + 1;
  }
};

template <int kP>
__global__ __launch_bounds__(kIngestBlock) void spectator_ingest_kernel(SpecIngestParams p) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];  // (IngestLane)
  const IngestLane b(p.feed, smem);
  SpecRows<kP> rows{p, b.s, b.live, p.feed.c0 % p.acap, 0};
  ingest_walk<kP>(p.feed, b, rows);
}

int ingest_launch(ggrs_spectator_engine* e, int32_t first_call, int32_t n, const int32_t* start_frame,
                  const int32_t* packet_len, const uint8_t* packets, const int32_t* notes) {
  SpecIngestParams p;
  const IngestPlan plan = ingest_plan(e->feed.stride, n, 0);
  p.feed = ingest_feed(e->feed, e->cfg.num_sessions, e->cap, e->pkt_maxp, first_call, n, plan.G, start_frame, packet_len,
                       packets);
  p.acap = e->acap;
  p.rows = e->rows;
  p.recv = reinterpret_cast<int32_t*>(e->recv);
  p.notes = reinterpret_cast<int32_t*>(e->notes);
  p.notes_in = notes;
  if (int rc = e->timer.before(e->stream)) return rc;
  const unsigned grid = (unsigned)grid_of(p.feed.S, kIngestBlock);
  dispatch_players(e->cfg.num_players, [&](auto PC) {
    constexpr int PP = decltype(PC)::value;
    spectator_ingest_kernel<PP><<<grid, kIngestBlock, plan.lds, e->stream>>>(p);
  });
  HIP_TRY(hipGetLastError());
  e->timer.count();
  return GGRS_OK;
}

}  // namespace

namespace ggrs {

int spectator_ingest_free(ggrs_spectator_engine* e) {
  e->feed.release();
  return GGRS_OK;
}

}  // namespace ggrs

extern "C" {

int ggrs_spectator_set_packet_feed(ggrs_spectator_engine_t* e, int32_t max_prediction, int32_t max_packet_inputs,
                                   int32_t packet_stride) {
  if (!e) return set_error(GGRS_E_INVALID, "null engine");
  if (e->calls != 0 || e->next_arrival_call != 0 || e->next_input_frame != 0)
    return set_error(GGRS_E_STATE, "the packet feed is part of the engine's configuration (set before the first input, "
                     "arrival and call)");
  if (max_prediction < 0) return set_error(GGRS_E_INVALID, "max_prediction must be >= 0, got %d", max_prediction);
  if (int rc = PacketFeedState::check(e->cfg.num_players, max_packet_inputs, packet_stride, kIngestMaxStride)) return rc;
  if ((int64_t)e->cap <= 2 * (int64_t)max_prediction + max_packet_inputs)
    return set_error(GGRS_E_INVALID, "input_capacity %d must exceed 2 * max_prediction + max_packet_inputs = %lld (a packet "
                     "must not reach its own reference's row slot)", e->cap,
                     (long long)(2 * (int64_t)max_prediction + max_packet_inputs));
  HIP_TRY(hipSetDevice(e->cfg.device));
  if (int rc = e->feed.reset((size_t)e->cfg.num_sessions, (size_t)e->cap, max_packet_inputs, packet_stride, e->stream))
    return rc;
  e->pkt = 1;
  e->pkt_maxp = max_prediction;
  return GGRS_OK;
}

int ggrs_spectator_receive_packets(ggrs_spectator_engine_t* e, int32_t first_call, int32_t n, const int32_t* start_frame,
                                   const int32_t* packet_len, const uint8_t* packets, const int32_t* notes,
                                   int32_t on_device) {
  if (!e) return set_error(GGRS_E_INVALID, "null engine");
  if (!e->pkt) return set_error(GGRS_E_STATE, "receiving packets needs ggrs_spectator_set_packet_feed");
  if (n < 0) return set_error(GGRS_E_INVALID, "n_calls must be >= 0");
  if (first_call != e->next_arrival_call)
    return set_error(GGRS_E_INVALID, "packets must be received in call order (expected call %d, got %d)",
                     e->next_arrival_call, first_call);
  if (n == 0) return GGRS_OK;
  if (!start_frame || !packet_len || !packets) return set_error(GGRS_E_INVALID, "null argument");
  if ((int64_t)first_call + n - 1 - e->calls >= e->cap)
    return set_error(GGRS_E_INVALID, "arrival queue full (capacity %d calls)", e->cap);
  if (on_device && ((uintptr_t)packets & 3)) return set_error(GGRS_E_INVALID, "device packets must be dword aligned");
  const size_t S = (size_t)e->cfg.num_sessions, rows = (size_t)n * S;
  if (notes && !on_device) {
    const int P = e->cfg.num_players;
    for (size_t i = 0; i < rows; i++) {
      const int32_t v = notes[i];
      if (v == 0) continue;
      if (!(v & 1) || v < 0 || ((v >> 1) & 3) >= P)
        return set_error(GGRS_E_INVALID, "bad connect-status note %d (call %d, session %lld): GGRS_SPECTATOR_NOTE(player, "
                         "frame) of one of the session's players, frame >= -1", v, first_call + (int32_t)(i / S),
                         (long long)(i % S));
    }
  }
  HIP_TRY(hipSetDevice(e->cfg.device));
  if (!on_device)  // through the feed's staging buffer, the calls' notes beside them
    if (int rc = e->feed.stage(rows, &start_frame, &packet_len, &packets, &notes, e->stream)) return rc;
  if (int rc = ingest_launch(e, first_call, n, start_frame, packet_len, packets, notes)) return rc;
  // host sources: the caller may reuse its arrays on return (as ggrs_spectator_add_arrivals); device
  // sources are read in stream order, nothing to wait for
  if (!on_device) HIP_TRY(hipStreamSynchronize(e->stream));
  e->next_arrival_call = first_call + n;
  return GGRS_OK;
}

int ggrs_spectator_read_packet_results(ggrs_spectator_engine_t* e, int32_t first_call, int32_t n, int32_t* status,
                                       int32_t* ack_frame) {
  if (!e) return set_error(GGRS_E_INVALID, "null engine");
  if (!e->pkt) return set_error(GGRS_E_STATE, "packet results exist with ggrs_spectator_set_packet_feed only");
  HIP_TRY(hipSetDevice(e->cfg.device));
  return e->feed.read(first_call, n, e->next_arrival_call, e->cap, e->cfg.num_sessions, status, ack_frame, e->stream);
}

}  // extern "C"
