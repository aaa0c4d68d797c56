// p2p_engine.h -- the P2P engine object shared by p2p.hip (fixed-latency network: every kernel form,
// desync detection, lockstep) and p2p_sched.hip (scheduled arrivals: per-session remote-arrival
// tables, the prediction threshold and disconnects) and p2p_ingest.hip (the packet feed of the
// scheduled mode) and p2p_emit.hip (its send side) and p2p_spec_emit.hip (the send side towards the
// sessions' spectators).  Host-side only; no kernels here.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "common.h"
#include "p2p_plan.h"

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
  int32_t emit = 0;                 // the mode
  int32_t emit_max = 0;             // max_pending_inputs
  int32_t emit_stride = 0;          // bytes per emitted packet row
  int32_t emit_next = 0;            // the next call to emit
  int32_t* emit_ll = nullptr;       // [cap][S] per call: the local players' last queued frame after it, or
                                    // kEmitStopped from the call that stopped the session (the scheduled kernels write it)
  uint32_t* emit_ring = nullptr;    // [kEmitPending][S] pending_output, slot frame % kEmitPending
  int32_t* emit_st = nullptr;       // [kEmitFields][S] the endpoint's send-side words (EmitField)
  uint8_t* emit_staging = nullptr;  // host-sourced calls: acks, resend flags and the outputs
  size_t emit_staging_bytes = 0;
  // spectator emit (ggrs_p2p_set_spectator_emit; p2p_spec_emit.hip): the sessions' confirmed inputs as
  // Input messages to their spectators, spec_k endpoints per session; reads emit_ll as packet emit does
  int32_t spec = 0;                 // the mode
  int32_t spec_k = 0;               // spectator endpoints per session
  int32_t spec_max = 0;             // max_pending_inputs
  int32_t spec_stride = 0;          // bytes per emitted packet row
  int32_t spec_q = 0;               // frames of the confirmed-input ring (2^k)
  int32_t spec_next = 0;            // the next call to emit
  uint32_t* spec_ring = nullptr;    // [spec_q][S] every player's confirmed byte of frame f, slot f & (spec_q - 1)
  int32_t* spec_st = nullptr;       // [kSpecFields][S] the session's words (SpecField)
  int32_t* spec_ep = nullptr;       // [kSpecEpFields][spec_k][S] the endpoints' words (SpecEpField)
  uint8_t* spec_staging = nullptr;  // host-sourced calls: acks, resend flags and the outputs
  size_t spec_staging_bytes = 0;
  ggrs::SpanTimer timer;
};

namespace ggrs {
// packet emit: PENDING_OUTPUT_SIZE (protocol.rs:22); the mark of a stopped session in emit_ll; the
// per-session words kept between launches
constexpr int kEmitPending = 128;
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
// p2p_emit.hip: free packet emit's buffers and emit_ll (the engine's destruction: after p2p_spec_emit_free)
int p2p_emit_free(ggrs_p2p_engine* e);
// p2p_spec_emit.hip: free spectator emit's own buffers (emit_ll is p2p_emit_free's)
int p2p_spec_emit_free(ggrs_p2p_engine* e);
// emit_ll, shared by the two emits: allocated by the first configured, every row "nothing queued"
int p2p_emit_ll_alloc(ggrs_p2p_engine* e);
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
