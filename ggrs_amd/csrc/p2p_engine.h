// p2p_engine.h -- the P2P engine object shared by p2p.hip (fixed-latency network: every kernel form,
// desync detection, lockstep) and p2p_sched.hip (scheduled arrivals: per-session remote-arrival
// tables, the prediction threshold and disconnects) and p2p_ingest.hip (the packet feed of the
// scheduled mode) and p2p_emit.hip (its send side) and p2p_spec_emit.hip (the send side towards the
// sessions' spectators), p2p_time_sync.hip and p2p_desync.hip (time sync and the checksum comparison,
// which walk the same calls by the same order rule) and p2p_poll.hip (the endpoint poll, which walks the
// calls before they run) and p2p_events.hip (the sessions' event queues), with the host side the two send sides share (PacketEmitState: configuration
// and call-order checks, the staging of a launch's arrays, the group plan; emit_begin / emit_end: an
// emit call before and after the unit's kernel launch; EmitCalls: what emit_begin hands the unit for
// its kernel's parameters).  Host code and plain structs only; no kernels here.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "codec_device.h"
#include "common.h"
#include "events_host.h"
#include "p2p_plan.h"
#include "poll_host.h"

namespace ggrs {
// the two emits: PENDING_OUTPUT_SIZE (protocol.rs:22); the kernels' block (one wave of sessions), the
// packet rows per session built before a write-out (at most), and the LDS a block's rows of one group
// slot (and their lengths) must fit
constexpr int kEmitPending = 128;
constexpr int kEmitBlock = 64;
constexpr int kEmitGroup = 8;
constexpr size_t kEmitLds = 64 * 1024;

// The six arrays of an emit launch of n calls, K endpoints a session (packet emit: K = 1)
struct EmitIo {
  const int32_t* ack_in;  // [n][K][S] or null
  const uint8_t* resend;  // [n][K][S] or null
  int32_t* start;         // [n][K][S]
  int32_t* len;           // [n][K][S]
  int32_t* word;          // [n][S] the per-call word: packet emit's ack_frame, spectator emit's notes
  uint8_t* packets;       // [n][K][S][stride]
};

// The host side of an emit (ggrs_p2p_set_packet_emit, ggrs_p2p_set_spectator_emit): its configuration,
// the next call to emit and the staging buffer of host-sourced calls; embedded twice in the engine.
struct PacketEmitState {
  int32_t on = 0;           // the mode
  int32_t max_pending = 0;  // max_pending_inputs
  int32_t stride = 0;       // bytes per emitted packet row
  int32_t next = 0;         // the next call to emit
  uint8_t* staging = nullptr;  // host-sourced calls: acks, resend flags and the outputs
  size_t staging_bytes = 0;

  // LDS of one group slot: a block's packet rows and their lengths
  static size_t slot_bytes(int32_t stride) { return (size_t)kEmitBlock * (odd_dword_pitch(stride) + sizeof(int32_t)); }
  // max_pending_inputs and out_stride for pending inputs of `bytes` bytes
  static int check(int bytes, int32_t max_pending_inputs, int32_t out_stride) {
    if (max_pending_inputs < 1 || max_pending_inputs > kEmitPending)
      return set_error(GGRS_E_INVALID, "max_pending_inputs must be in 1..%d (PENDING_OUTPUT_SIZE), got %d", kEmitPending,
                       max_pending_inputs);
    const int32_t need = ggrs_codec_max_packet_bytes(bytes, max_pending_inputs);
    if (out_stride < need || out_stride % 4)
      return set_error(GGRS_E_INVALID, "out_stride must be a multiple of 4 and >= ggrs_codec_max_packet_bytes(%d, %d) = %d, got %d",
                       bytes, max_pending_inputs, need, out_stride);
    if (out_stride > 1012 || slot_bytes(out_stride) > kEmitLds)
      return set_error(GGRS_E_INVALID, "out_stride %d is too long (at most 1012)", out_stride);
    return GGRS_OK;
  }
  void configure(int32_t max_pending_inputs, int32_t out_stride) {
    on = 1;
    max_pending = max_pending_inputs;
    stride = out_stride;
    next = 0;
  }
  // An emit call's order and arguments: calls first_call .. first_call + n - 1 of current_frame calls
  // run, the input rows held from call oldest_held on (the last cap).  n == 0 is GGRS_OK with nothing
  // to launch.
  int check_calls(int32_t first_call, int32_t n, int32_t current_frame, int32_t oldest_held, int32_t cap, const EmitIo& io,
                  int32_t on_device) const {
    if (int rc = check_order(first_call, n, current_frame, oldest_held, cap, !io.start || !io.len || !io.word || !io.packets))
      return rc;
    if (n > 0 && on_device && ((uintptr_t)io.packets & 3))
      return set_error(GGRS_E_INVALID, "device packets must be dword aligned");
    return GGRS_OK;
  }
  // ... the order alone (time sync, p2p_time_sync.hip, walks the same calls by the same rule): null_arg
  // says an output array is missing, `what` names the caller in the order error
  int check_order(int32_t first_call, int32_t n, int32_t current_frame, int32_t oldest_held, int32_t cap, bool null_arg,
                  const char* what = "packets are emitted") const {
    if (n < 0) return set_error(GGRS_E_INVALID, "n_calls must be >= 0");
    if (first_call != next)
      return set_error(GGRS_E_INVALID, "%s in call order, each call once (expected call %d, got %d)", what, next, first_call);
    if (n == 0) return GGRS_OK;
    if (null_arg) return set_error(GGRS_E_INVALID, "null argument");
    if ((int64_t)first_call + n > current_frame)
      return set_error(GGRS_E_INVALID, "calls up to %d are emitted after they ran (%d calls run)", first_call + n - 1,
                       current_frame);
    if (first_call < oldest_held)
      return set_error(GGRS_E_INVALID, "call %d is no longer held (the last %d calls' rows are)", first_call, cap);
    return GGRS_OK;
  }
  // The arrays the kernel takes for the caller's `io`: the caller's own when they are on the device,
  // else the staging buffer's, [ack_in][start][len][word][packets][resend], the two inputs uploaded
  // where given (stream order keeps an earlier launch's use of the buffer ahead of the copies).
  int begin(const EmitIo& io, size_t n, size_t K, size_t S, int32_t on_device, hipStream_t stream, EmitIo* dev) {
    *dev = io;
    if (on_device) return GGRS_OK;
    const size_t rows = n * K * S, calls = n * S;
    if (int rc = grow_staging(&staging, &staging_bytes, rows * (12 + (size_t)stride + 1) + 4 * calls)) return rc;
    int32_t* d_ack_in = reinterpret_cast<int32_t*>(staging);
    dev->start = d_ack_in + rows;
    dev->len = dev->start + rows;
    dev->word = dev->len + rows;
    dev->packets = reinterpret_cast<uint8_t*>(dev->word + calls);
    uint8_t* d_resend = dev->packets + rows * (size_t)stride;
    if (io.ack_in) HIP_TRY(hipMemcpyAsync(d_ack_in, io.ack_in, 4 * rows, hipMemcpyHostToDevice, stream));
    if (io.resend) HIP_TRY(hipMemcpyAsync(d_resend, io.resend, rows, hipMemcpyHostToDevice, stream));
    dev->ack_in = io.ack_in ? d_ack_in : nullptr;
    dev->resend = io.resend ? d_resend : nullptr;
    return GGRS_OK;
  }
  // ... and after the launch: the staged outputs back into the caller's, waited for
  int end(const EmitIo& io, const EmitIo& dev, size_t n, size_t K, size_t S, int32_t on_device, hipStream_t stream) const {
    if (on_device) return GGRS_OK;
    const size_t rows = n * K * S;
    HIP_TRY(hipMemcpyAsync(io.start, dev.start, 4 * rows, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipMemcpyAsync(io.len, dev.len, 4 * rows, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipMemcpyAsync(io.word, dev.word, 4 * n * S, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipMemcpyAsync(io.packets, dev.packets, rows * (size_t)stride, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return GGRS_OK;
  }
  // The group slots built before a write-out and the launch's dynamic LDS, for n calls of
  // slots_per_call (call, endpoint) pairs: up to kEmitGroup calls' slots, as many as fit the LDS
  // budget, which keeps two blocks on a CU at every stride
  struct Group { int32_t G; size_t lds; };
  Group group(size_t slots_per_call, size_t n) const {
    const size_t per_slot = slot_bytes(stride);
    const size_t G = std::max<size_t>(1, std::min<size_t>({kEmitGroup * slots_per_call, kEmitLds / per_slot, n * slots_per_call}));
    return {(int32_t)G, G * per_slot};
  }
  void release() {
    if (staging) (void)hipFree(staging);
    staging = nullptr;
    staging_bytes = 0;
    on = 0;
  }
};

// Field f of a [fields][rows] device array into a host array, if one is given
inline hipError_t read_field(int32_t* dst, const int32_t* fields, int f, size_t rows, hipStream_t stream) {
  return dst ? hipMemcpyAsync(dst, fields + (size_t)f * rows, 4 * rows, hipMemcpyDeviceToHost, stream) : hipSuccess;
}
}  // namespace ggrs

struct ggrs_p2p_engine {
  ggrs_p2p_config_t cfg{};
  int Pp = 1, F = 1, R = 2, cap = 256;
  int num_cus = 256;                 // the device's CUs (LDS-ring occupancy rule)
  hipStream_t stream = nullptr;
  uint32_t* cur = nullptr;
  uint32_t* ring = nullptr;
  uint8_t* inputs = nullptr;
  int32_t* queue = nullptr;
  int32_t* rollbacks = nullptr;
  int64_t* resim = nullptr;
  uint16_t* trace = nullptr;
  uint8_t* staging = nullptr;
  size_t staging_bytes = 0;
  int32_t current_frame = 0;         // advance_frame calls made (the session frame in rollback mode
                                     // with a fixed latency; per session in scheduled mode)
  int32_t next_input_frame = 0;
  int32_t desync_interval = 0;
  uint16_t* hist = nullptr;     // [kHist][S] local checksum history
  uint64_t* cmp_mask = nullptr; // [ceil(S/64)] compare result
  int32_t* cmp_count = nullptr;
  int64_t dbg_sess = -1;
  int32_t dbg_frame = -1;
  int32_t sparse = 0;
  ggrs::P2PForm form = ggrs::P2PForm::kDefault;  // ggrs_p2p_set_unstaged (the forms: kP2PForms, p2p_plan.h)
  bool dbg_ever = false;  // a debug flip was armed: the states may no longer be the canonical ones
  int32_t* last_saved = nullptr;  // [S], sparse saving only
  int32_t* ring_frame = nullptr;  // [R][S]: the frame each cell holds (sparse saving, scheduled mode)
  // lockstep mode (max_prediction 0): the session-uniform control flow, replayed on the host
  int32_t ls_frame = 0;                     // SyncLayer::current_frame
  int32_t ls_local_last = GGRS_NULL_FRAME;  // local players' last queue frame (local_connect_status)
  std::vector<int32_t> ls_row_of;           // queue frame q -> the call (input row) that added it, q % size
  int32_t* ls_prog = nullptr;               // device copy of a launch's (local row, remote row) pairs
  int32_t ls_prog_cap = 0;
  // scheduled arrivals (ggrs_p2p_set_arrival_schedule; p2p_sched.hip)
  int32_t sched = 0;
  int32_t next_arrival_call = 0;
  int32_t* arrive = nullptr;      // [cap][S] newest remote frame delivered by call c, row c % cap
  uint8_t* events = nullptr;      // [cap][S] Event::Disconnected bits of call c
  int32_t* peer_reports = nullptr;  // [cap][S] the peers' disconnect reports of call c (ggrs_p2p_add_peer_reports)
  int32_t* row_tag = nullptr;     // [cap] the frame whose input row each row slot holds
  std::vector<int32_t> row_tag_host;
  uint32_t* iq = nullptr;         // [kSchedQueue][S] every player's queued input of frame q, q % kSchedQueue
  int32_t* sst = nullptr;         // [sched_fields(P)][S] SyncLayer / InputQueue / connect-status words
  // scheduled desync detection: per call (row c % cap) the report sent, its checksum, the
  // last_confirmed_frame compared against, the last queued local frame; every frame's final cell
  // checksum [sched_hf][S]
  int32_t* rep_frame = nullptr;
  uint16_t* rep_ck = nullptr;
  int32_t* rep_lconf = nullptr;
  int32_t* rep_ll = nullptr;
  uint16_t* fck = nullptr;
  int32_t sched_hf = 0;
  // packet feed (ggrs_p2p_set_packet_feed; p2p_ingest.hip): the remote inputs enter as the wire
  // packets each call's poll received, and the device writes the arrival table
  int32_t pkt = 0;                 // the mode
  ggrs::PacketFeedState feed;      // (stop: see p2p_ingest.hip; staged beside the packets: the calls' events)
  // packet emit (ggrs_p2p_set_packet_emit; p2p_emit.hip): the sessions' outgoing Input messages
  ggrs::PacketEmitState emit;
  int32_t* emit_ll = nullptr;       // [cap][S] per call: the local players' last queued frame after it, or
                                    // kEmitStopped from the call that stopped the session (the scheduled kernels write it)
  uint32_t* emit_ring = nullptr;    // [kEmitPending][S] pending_output, slot frame % kEmitPending
  int32_t* emit_st = nullptr;       // [kEmitFields][S] the endpoint's send-side words (EmitField)
  // spectator emit (ggrs_p2p_set_spectator_emit; p2p_spec_emit.hip): the sessions' confirmed inputs as
  // Input messages to their spectators, spec_k endpoints per session; reads emit_ll as packet emit does
  ggrs::PacketEmitState spec;
  int32_t spec_k = 0;               // spectator endpoints per session
  int32_t spec_q = 0;               // frames of the confirmed-input ring (2^k)
  uint32_t* spec_ring = nullptr;    // [spec_q][S] every player's confirmed byte of frame f, slot f & (spec_q - 1)
  int32_t* spec_st = nullptr;       // [kSpecFields][S] the session's words (SpecField)
  int32_t* spec_ep = nullptr;       // [kSpecEpFields][spec_k][S] the endpoints' words (SpecEpField)
  // time sync (ggrs_p2p_set_time_sync; p2p_time_sync.hip): the endpoint's TimeSync windows, frames_ahead and
  // the wait recommendation per call; reads emit_ll as the two emits do (tsync: the mode, the next call
  // and the staging of host-sourced calls -- its max_pending and stride are unused)
  ggrs::PacketEmitState tsync;
  int32_t tsync_fps = 0;
  int32_t* tsync_win = nullptr;     // [2][kTsWindow][S] the local and the remote window
  int32_t* tsync_st = nullptr;      // [kTsFields][S] the endpoint's time-sync words (TsField)
  // checksum comparison (ggrs_p2p_set_desync_compare; p2p_desync.hip): the peer's report rows, the two
  // tables of UdpProtocol::on_checksum_report and compare_local_checksums_against_peers, the events
  // (dcmp: the mode and the next call -- its staging holds host-sourced peer rows)
  ggrs::PacketEmitState dcmp;
  int32_t dcmp_interval = 0;        // the interval it was configured with
  int32_t dcmp_max_events = 0;
  int32_t dcmp_added = 0;           // the peer's rows added so far
  int32_t* dcmp_peer_frame = nullptr;  // [cap][S] the peer's report rows, row g % cap: the frame (-1 none),
  uint16_t* dcmp_peer_ck = nullptr;    // ... its checksum
  int32_t* dcmp_peer_ll = nullptr;     // ... and the peer's last queued local frame after its call g
  int32_t* dcmp_frames = nullptr;   // [2][kDcTable][S] local_checksum_history's then pending_checksums' frames
  uint16_t* dcmp_cks = nullptr;     // [2][kDcTable][S] ... and checksums
  int32_t* dcmp_st = nullptr;       // [kDcFields][S] the session's words (DcField)
  int32_t* dcmp_events = nullptr;   // [4][max_events] call, session, frame, local | remote << 16
  unsigned long long* dcmp_count = nullptr;  // the events raised (exact past max_events)
  hipEvent_t dcmp_sync[2] = {nullptr, nullptr};  // ggrs_p2p_add_remote_reports_from: the two streams' order
  // endpoint poll (ggrs_p2p_set_endpoint_poll; p2p_poll.hip): UdpProtocol::poll's timers, the disconnect
  // timeout and the endpoint's state per call, before the call runs
  int32_t endp_on = 0;              // the mode
  int32_t endp_next = 0;            // the next call to poll
  uint8_t* endp_staging = nullptr;  // host-sourced calls: the clocks, kinds and the outputs
  size_t endp_staging_bytes = 0;
  uint64_t endp_timeout = 0, endp_notify = 0;  // disconnect_timeout, disconnect_notify_start (ms)
  uint64_t endp_host_clock = 0;     // the last clock a host array gave (a host array never goes below it)
  int32_t endp_launches = 0;        // launch i reads endp_clock[i & 1] and writes endp_clock[(i + 1) & 1]
  uint64_t* endp_times = nullptr;   // [kPollTimes][S] the endpoint's Instants (PollTime)
  int32_t* endp_st = nullptr;       // [kPollFields][S] its flag word and closing call (PollField)
  uint64_t* endp_clock = nullptr;   // [2] the engine's last clock
  // spectator endpoint poll (ggrs_p2p_set_spectator_poll; p2p_spec_poll.hip): the same for the spec_k
  // endpoints a session has towards its spectators, [..][spec_k][S] rows; spectator emit reads its
  // closed_call row
  ggrs::PollHost spoll;
  // event queue (ggrs_p2p_set_event_queue; p2p_events.hip): every session's GgrsEvent queue, filled per call
  // from the polls', time sync's and the comparison's outputs, drained into one list
  ggrs::EventQueueHost evq;
  ggrs::SpanTimer timer;
};

namespace ggrs {
// packet emit: the mark of a stopped session in emit_ll; the per-session words kept between launches
constexpr int32_t kEmitStopped = INT32_MIN;
enum EmitField : int {
  kEmitLaFrame = 0,  // last_acked_input: its frame
  kEmitLaBytes,      // ... and bytes
  kEmitHead,         // the first pending frame (while any is pending)
  kEmitCount,        // pending inputs
  kEmitStatus,       // 0 open, GGRS_EMIT_CLOSED, GGRS_EMIT_DISCONNECTED
  kEmitClosedCall,   // the call that closed the stream (-1)
  kEmitLlPrev,       // the local players' last queued frame after the last emitted call
  kEmitRecv,         // the endpoint's last_recv_frame after it
  kEmitFields
};
// spectator emit: the session's words and each endpoint's, kept between launches
enum SpecField : int {
  kSpecNext = 0,   // next_spectator_frame
  kSpecLlPrev,     // the local players' last queued frame after the last emitted call
  kSpecRecv,       // the newest remote frame delivered by it
  kSpecDisc,       // the disconnected players' mask
  kSpecLostCall,   // the call that found an input row lost (-1)
  kSpecLf0,        // [4] a disconnected player's frozen last frame
  kSpecFields = kSpecLf0 + 4
};
enum SpecEpField : int {
  kSpecEpLaFrame = 0,  // last_acked_input: its frame
  kSpecEpLaBytes,      // ... and bytes
  kSpecEpPending,      // pending inputs after the last emitted call
  kSpecEpStatus,       // 0 open, GGRS_EMIT_DISCONNECTED, GGRS_EMIT_ROW_LOST
  kSpecEpClosedCall,   // the call that closed the endpoint (-1)
  kSpecEpFields
};
// time sync: FRAME_WINDOW_SIZE (time_sync.rs:3); the per-session words kept between launches
constexpr int kTsWindow = 30;
enum TsField : int {
  kTsRtt = 0,      // round_trip_time, ms
  kTsRemote,       // remote_frame_advantage
  kTsLocal,        // local_frame_advantage
  kTsNextSleep,    // next_recommended_sleep
  kTsClosedCall,   // the call that closed the endpoint (-1: open)
  kTsLlPrev,       // the local players' last queued frame after the last call taken
  kTsRecv,         // the endpoint's last_recv_frame after it
  kTsFields
};
// checksum comparison: MAX_CHECKSUM_HISTORY_SIZE (protocol.rs:27); the per-session words kept between launches
constexpr int kDcTable = 32;
enum DcField : int {
  kDcCursor = 0,   // the peer's rows delivered so far
  kDcNewest,       // the newest frame received from the peer (NULL_FRAME)
  kDcRecv,         // the endpoint's last_recv_frame after the last call compared
  kDcStatus,       // 0, GGRS_DESYNC_ROW_LOST
  kDcHist,         // entries of local_checksum_history
  kDcPend,         // entries of pending_checksums
  kDcRefused,      // reports refused
  kDcEvents,       // DesyncDetected events raised
  kDcFirstCall,    // the first event's call (-1), frame (-1), local and remote checksum
  kDcFirstFrame,
  kDcFirstLocal,
  kDcFirstRemote,
  kDcFields
};
// p2p_events.hip: free the event queue's buffers
int p2p_events_free(ggrs_p2p_engine* e);
// p2p_poll.hip: free the endpoint poll's buffers
int p2p_poll_free(ggrs_p2p_engine* e);
// p2p_spec_poll.hip: free the spectator endpoint poll's buffers (and turn it off)
int p2p_spec_poll_free(ggrs_p2p_engine* e);
// p2p_desync.hip: free the checksum comparison's buffers
int p2p_desync_free(ggrs_p2p_engine* e);
// p2p_time_sync.hip: free time sync's own buffers (emit_ll is p2p_emit_free's)
int p2p_time_sync_free(ggrs_p2p_engine* e);
// p2p_emit.hip: free packet emit's buffers and emit_ll (the engine's destruction: after p2p_spec_emit_free)
int p2p_emit_free(ggrs_p2p_engine* e);
// p2p_spec_emit.hip: free spectator emit's own buffers (emit_ll is p2p_emit_free's)
int p2p_spec_emit_free(ggrs_p2p_engine* e);
// emit_ll, shared by the two emits and time sync: allocated by the first configured, every row "nothing queued"
int p2p_emit_ll_alloc(ggrs_p2p_engine* e);

// What an emit kernel's parameters take from the engine for a launch of calls c0 .. c0 + n - 1: the
// rows the scheduled kernels and the feed left, the emit's configuration and the launch's arrays
// (device pointers)
struct EmitCalls {
  int64_t S;
  int32_t cap, c0, n;
  int32_t G;               // group slots (PacketEmitState::group)
  int32_t maxpend, stride, Pp, pkt;
  const uint8_t* inputs;   // [cap][S] row words
  const int32_t* ll;       // [cap][S] the local players' last queued frame after the call, or kEmitStopped
  const int32_t* arrive;   // [cap][S] (the packet feed off)
  const int32_t* pkt_ack;  // [cap][S] (the packet feed on)
  const uint8_t* events;   // [cap][S]
  EmitIo io;
};

// An emit call of either kind, of K endpoints a session over the engine's `st`.  emit_begin: the
// call-order checks, then (n > 0) the staging, *c filled and the launch's dynamic LDS bytes; the unit
// launches its kernel on grid_of(c->S, kEmitBlock) blocks; emit_end: the copy back, the call counted.
inline int emit_begin(ggrs_p2p_engine* e, PacketEmitState& st, size_t K, const EmitIo& io, int32_t first_call, int32_t n,
                      int32_t on_device, EmitCalls* c, size_t* lds) {
  const int32_t oldest_held = std::max(e->next_input_frame, e->next_arrival_call) - e->cap;
  if (int rc = st.check_calls(first_call, n, e->current_frame, oldest_held, e->cap, io, on_device)) return rc;
  if (n == 0) return GGRS_OK;
  HIP_TRY(hipSetDevice(e->cfg.device));
  const auto grp = st.group(K, n);
  *c = {e->cfg.num_sessions, e->cap, first_call, n, grp.G, st.max_pending, st.stride, e->Pp, e->pkt, e->inputs,
        e->emit_ll, e->arrive, e->feed.ack, e->events, {}};
  *lds = grp.lds;
  if (int rc = st.begin(io, n, K, (size_t)c->S, on_device, e->stream, &c->io)) return rc;
  return e->timer.before(e->stream);
}
inline int emit_end(ggrs_p2p_engine* e, PacketEmitState& st, size_t K, const EmitIo& io, const EmitCalls& c, int32_t on_device) {
  HIP_TRY(hipGetLastError());
  e->timer.count();
  if (int rc = st.end(io, c.io, c.n, K, (size_t)c.S, on_device, e->stream)) return rc;
  st.next = c.c0 + c.n;
  return GGRS_OK;
}
// p2p_sched.hip: enable scheduled mode (allocate and initialise its buffers), run n calls, upload arrival rows
int p2p_sched_enable(ggrs_p2p_engine* e);
int p2p_sched_advance(ggrs_p2p_engine* e, int32_t n);
int p2p_sched_free(ggrs_p2p_engine* e);
int p2p_sched_desync_alloc(ggrs_p2p_engine* e);  // desync detection's buffers (scheduled mode)
int32_t* p2p_sched_errors(ggrs_p2p_engine* e);    // [S] the sessions' errors (device)
// p2p_ingest.hip (packet feed): decode n calls' packets (device pointers, [n][S] rows) into the input
// rows and write their arrival rows; after a launch of calls, give the sessions the feed stopped in
// those calls their error; free the feed's buffers
int p2p_ingest_launch(ggrs_p2p_engine* e, int32_t first_call, int32_t n, const int32_t* start_frame,
                      const int32_t* packet_len, const uint8_t* packets, const uint8_t* events);
int p2p_ingest_after_advance(ggrs_p2p_engine* e);
int p2p_ingest_free(ggrs_p2p_engine* e);
}  // namespace ggrs
