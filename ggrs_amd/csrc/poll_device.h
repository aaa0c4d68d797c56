// poll_device.h -- one endpoint's poll step and the launch loop around it, shared by the three units
// that run UdpProtocol's timers on the device: p2p_poll.hip (the P2P engine's endpoint towards its remote
// players), p2p_spec_poll.hip (its endpoints towards its spectators) and spectator_poll.hip (the
// spectator engine's endpoint towards its host).  The step is UdpProtocol::poll
// (src/network/protocol.rs:329-376), the clock bookkeeping of handle_message (:534-551), on_input's
// running_last_input_recv and send_input_ack (:608, :634) and the owner's reaction to
// Event::Disconnected, over one clock per poll.  That reaction is what differs between the three owners
// of an endpoint, and it is a compile-time property of the step (PollOwner).  All times are u64
// milliseconds; every comparison is strict, as the reference's are.
//
// send_keep_alive (:344-347) is not here because it cannot fire: last_send_time is set by every
// queue_message, send_quality_report sets running_last_quality_report and then queues, and the
// constructor initialises the two in that order, so last_send_time >= running_last_quality_report at
// every check; both intervals are 200 ms, so either the report fired in this poll (last_send_time is
// then later than poll's `now`) or last_send_time + 200 >= running_last_quality_report + 200 >= now
// (DESIGN.md section 3 "Endpoint poll"; tests/test_endpoint_poll_model.py pins it on a literal model).
// The argument does not depend on who the peer is: no owner has a keep-alive row.
//
// The launch loop (poll_walk): one thread per endpoint, one wave per block; the launch's calls are
// walked in order because the times carry from call to call.  The four times and the flag word live in
// registers for the launch, loaded from and stored to [fields][E] rows.  The clock of a call is
// wave-uniform: now_ms and the engine's last clock come through the scalar path.  A group of calls'
// input bytes is loaded before its first use; the outputs are coalesced [E] byte stores.  No LDS, no
// scratch.  The last clock is kept in device memory in two slots, read from one and written to the
// other by alternate launches: a block that starts late must not read what the first block already
// wrote.  What a unit reads per call and what it does with a raised Event::Disconnected is its Io.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ggrs_amd.h"
#include "poll_host.h"

namespace ggrs {

constexpr int kPollBlock = 64;  // one wave of endpoints
constexpr int kPollGroup = 8;   // calls whose input bytes are loaded together, ahead of their steps

constexpr uint64_t kPollRetryMs = 200;      // RUNNING_RETRY_INTERVAL (protocol.rs:17)
constexpr uint64_t kPollReportMs = 200;     // QUALITY_REPORT_INTERVAL (:19)
constexpr uint64_t kPollShutdownMs = 5000;  // UDP_SHUTDOWN_TIMER (:21)
// the endpoint's flag word: disconnect_notify_sent, disconnect_event_sent, then ProtocolState
constexpr uint32_t kPollNotifySent = 1, kPollEventSent = 2;
constexpr int kPollStateShift = kPollWordStateShift;
// what a step returns beside the GGRS_NET_* bits (bits 0-3)
constexpr uint32_t kPollResend = 16, kPollSendAck = 32, kPollSendReport = 64;
// a step's `ext`: an Event::Disconnected from outside poll() is to be handled at this call; with
// kPollExtEvent it is one the owner's event loop sees (GGRS_NET_DISCONNECTED), else it is silent
constexpr uint32_t kPollExt = 1, kPollExtEvent = 2;

// Who owns the endpoint, which decides what Event::Disconnected leads to:
enum class PollOwner : int {
  // P2PSession, a remote player's endpoint: disconnect_player_at_frame calls disconnect()
  // (p2p_session.rs:618-655).  ext is a received disconnect_requested (or the host's own), which sets
  // disconnect_event_sent (on_input, :569-574).
  kSessionRemote,
  // P2PSession, a spectator's endpoint: handle_event (:866-878) -> disconnect_player(spectator)
  // (:506-509) -> disconnect().  ext is the host's own disconnect_player or send_input's queued overflow
  // event (protocol.rs:443-445, kPollExtEvent); neither sets disconnect_event_sent.
  kSessionSpectator,
  // SpectatorSession, the host's endpoint: handle_event (p2p_spectator_session.rs:199-239) only
  // forwards GgrsEvent::Disconnected and never calls disconnect(), so the endpoint stays Running for
  // good: its timers and the interrupted / resumed pair go on, and disconnect_event_sent is all that
  // keeps the event from being raised twice.  ext is a received disconnect_requested.
  kSpectatorHost,
};

struct PollEndpoint {
  uint64_t last_recv;        // last_recv_time
  uint64_t last_input_recv;  // running_last_input_recv
  uint64_t last_report;      // running_last_quality_report
  uint64_t shutdown;         // shutdown_timeout
  uint32_t word;             // kPollNotifySent | kPollEventSent | state << kPollStateShift
  int32_t closed_call;       // the call at which the endpoint went Running -> Disconnected (kSpectatorHost:
                             // at which its one Event::Disconnected was raised) (-1)
};

// Call c's poll of one endpoint at clock `now`: any = a message was accepted, decoded = an Input
// among them was decoded, ext = kPollExt bits (see PollOwner).  Returns GGRS_NET_* | kPollResend |
// kPollSendAck | kPollSendReport.
template <PollOwner kOwner>
__device__ __forceinline__ uint32_t poll_endpoint_step(PollEndpoint& ep, uint64_t now, uint64_t timeout, uint64_t notify,
                                                       int32_t c, bool any, bool decoded, uint32_t ext) {
  const uint32_t state = ep.word >> kPollStateShift;
  if (state == GGRS_ENDPOINT_SHUTDOWN) return 0;  // 0. (:538-541, :373)
  uint32_t out = 0;
  if (any) {  // 1. handle_message (:544-551)
    ep.last_recv = now;
    if ((ep.word & kPollNotifySent) && state == GGRS_ENDPOINT_RUNNING) {
      ep.word &= ~kPollNotifySent;
      out |= GGRS_NET_RESUMED;
    }
  }
  if constexpr (kOwner == PollOwner::kSpectatorHost) {
    // on_input's disconnect_requested (:569-574): the event, once; the session only forwards it
    if (ext && !(ep.word & kPollEventSent)) {
      out |= GGRS_NET_DISCONNECTED;
      ep.word |= kPollEventSent;
      ep.closed_call = c;
    }
  }
  if (decoded) {  // 2. on_input (:608, :634)
    ep.last_input_recv = now;
    out |= kPollSendAck;
  }
  if (state == GGRS_ENDPOINT_RUNNING) {  // 4. poll (:332-367)
    if (ep.last_input_recv + kPollRetryMs < now) {
      out |= kPollResend;
      ep.last_input_recv = now;
    }
    if (ep.last_report + kPollReportMs < now) {
      out |= kPollSendReport;
      ep.last_report = now;
    }
    if (!(ep.word & kPollNotifySent) && ep.last_recv + notify < now) {
      out |= GGRS_NET_INTERRUPTED;
      ep.word |= kPollNotifySent;
    }
    if constexpr (kOwner == PollOwner::kSessionRemote)
      if (ext) ep.word |= kPollEventSent;  // (on_input's disconnect_requested, :569-574)
    if constexpr (kOwner == PollOwner::kSessionSpectator)
      if (ext & kPollExtEvent) out |= GGRS_NET_DISCONNECTED;  // (send_input's, drained by this poll)
    if (!(ep.word & kPollEventSent) && ep.last_recv + timeout < now) {
      out |= GGRS_NET_DISCONNECTED;
      ep.word |= kPollEventSent;
      if constexpr (kOwner == PollOwner::kSpectatorHost) ep.closed_call = c;
      ext |= kPollExt;
    }
    if constexpr (kOwner != PollOwner::kSpectatorHost) {
      if (ext) {  // the session handles the event: disconnect (:311-319)
        ep.word = (ep.word & ((1u << kPollStateShift) - 1u)) | (uint32_t)GGRS_ENDPOINT_DISCONNECTED << kPollStateShift;
        ep.shutdown = now + kPollShutdownMs;
        ep.closed_call = c;
      }
    }
  } else if (ep.shutdown < now) {  // 5. Disconnected at entry (:368-372)
    ep.word = (ep.word & ((1u << kPollStateShift) - 1u)) | (uint32_t)GGRS_ENDPOINT_SHUTDOWN << kPollStateShift;
    out |= GGRS_NET_SHUTDOWN;
  }
  return out;
}

// What every unit's launch takes: E endpoints, calls c0 .. c0 + n - 1
struct PollWalk {
  int64_t E;
  int32_t c0, n;
  uint64_t timeout, notify;
  const uint64_t* now;         // [n]
  const uint64_t* clock_in;    // the engine's last clock before the launch
  uint64_t* clock_out;         // ... and after it
  uint64_t* times;             // [kPollTimes][E]
  int32_t* st;                 // [kPollFields][E]
  uint8_t* o_resend;           // [n][E] each, or null
  uint8_t* o_ack;
  uint8_t* o_report;
  uint8_t* o_net;
};

// The launch loop of a poll kernel (kPollBlock threads a block, grid_of(E, kPollBlock) blocks).  Io is
// the unit's own part:
//   void begin(int64_t e)                                   per-launch words of endpoint e;
//   void load(int32_t k, int32_t c, int64_t e, uint32_t& kinds, uint32_t& ev, int32_t& status) const
//                                                            the launch's k-th call's (call c's) bytes;
//   bool decoded(uint32_t kinds, int32_t status) const       an Input among the messages was decoded;
//   uint32_t ext(uint32_t ev) const                          the step's ext;
//   void raised(int32_t c, int64_t e, uint32_t ev) const     the step raised GGRS_NET_DISCONNECTED.
template <PollOwner kOwner, class Io>
__device__ __forceinline__ void poll_walk(const PollWalk& p, Io io) {
  const int t = threadIdx.x;
  const int64_t E = p.E;
  const int64_t e0 = (int64_t)blockIdx.x * kPollBlock;
  const int nb = (int)min((int64_t)kPollBlock, E - e0);
  const bool live = t < nb;
  const int64_t e = live ? e0 + t : e0;  // idle lanes shadow the block's first endpoint, never store
  PollEndpoint ep;
  ep.last_recv = p.times[(int64_t)kPollLastRecv * E + e];
  ep.last_input_recv = p.times[(int64_t)kPollLastInputRecv * E + e];
  ep.last_report = p.times[(int64_t)kPollLastReport * E + e];
  ep.shutdown = p.times[(int64_t)kPollShutdown * E + e];
  ep.word = (uint32_t)p.st[(int64_t)kPollWord * E + e];
  ep.closed_call = p.st[(int64_t)kPollClosedCall * E + e];
  io.begin(e);
  uint64_t clock = *p.clock_in;

  for (int32_t k0 = 0; k0 < p.n; k0 += kPollGroup) {
    const int gn = min(kPollGroup, p.n - k0);
    // the group's per-call bytes, all loads in flight together (a short group repeats its last call)
    uint32_t kd8[kPollGroup], ev8[kPollGroup];
    int32_t st8[kPollGroup];
#pragma unroll
    for (int g = 0; g < kPollGroup; g++) {
      const int32_t k = k0 + min(g, gn - 1);
      io.load(k, p.c0 + k, e, kd8[g], ev8[g], st8[g]);
    }
    for (int g = 0; g < gn; g++) {
      const int32_t c = p.c0 + k0 + g;
      // an Instant never goes back: a clock below the engine's last is taken as that
      const uint64_t now = max(p.now[k0 + g], clock);
      clock = now;
      // this call's bytes: the front of the batch, which shifts down a call per iteration (indexing it
      // by g would put it in scratch memory)
      const uint32_t kd = kd8[0], ev = ev8[0];
      const int32_t status = st8[0];
#pragma unroll
      for (int j = 0; j < kPollGroup - 1; j++) {
        kd8[j] = kd8[j + 1];
        ev8[j] = ev8[j + 1];
        st8[j] = st8[j + 1];
      }
      const uint32_t r = poll_endpoint_step<kOwner>(ep, now, p.timeout, p.notify, c, kd != 0, io.decoded(kd, status), io.ext(ev));
      if (live) {
        const int64_t o = (int64_t)(k0 + g) * E + e;
        if (p.o_resend) p.o_resend[o] = (uint8_t)((r & kPollResend) != 0);
        if (p.o_ack) p.o_ack[o] = (uint8_t)((r & kPollSendAck) != 0);
        if (p.o_report) p.o_report[o] = (uint8_t)((r & kPollSendReport) != 0);
        if (p.o_net) p.o_net[o] = (uint8_t)(r & 15u);
        if (r & GGRS_NET_DISCONNECTED) io.raised(c, e, ev);
      }
    }
  }
  if (live) {
    p.times[(int64_t)kPollLastRecv * E + e] = ep.last_recv;
    p.times[(int64_t)kPollLastInputRecv * E + e] = ep.last_input_recv;
    p.times[(int64_t)kPollLastReport * E + e] = ep.last_report;
    p.times[(int64_t)kPollShutdown * E + e] = ep.shutdown;
    p.st[(int64_t)kPollWord * E + e] = (int32_t)ep.word;
    p.st[(int64_t)kPollClosedCall * E + e] = ep.closed_call;
  }
  if (blockIdx.x == 0 && t == 0) *p.clock_out = clock;
}

}  // namespace ggrs
