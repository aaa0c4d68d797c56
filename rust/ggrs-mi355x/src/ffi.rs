//! Hand-written declarations of every symbol in include/ggrs_amd.h (no bindgen: the ABI is plain
//! C).  tests/test_rust_ffi.py parses this file against the header -- names, parameter counts and
//! types, struct field order and types, constants -- so the two cannot drift apart.
#![allow(non_camel_case_types)]
use std::os::raw::{c_char, c_void};

pub const GGRS_ABI_VERSION: i32 = 6;

pub const GGRS_OK: i32 = 0;
pub const GGRS_E_INVALID: i32 = -1;
pub const GGRS_E_PRECONDITION: i32 = -2;
pub const GGRS_E_HIP: i32 = -3;
pub const GGRS_E_STATE: i32 = -4;
pub const GGRS_E_TOO_FAR_BEHIND: i32 = -5;

pub const GGRS_NULL_FRAME: i32 = -1;

pub const GGRS_REQ_SAVE: i32 = 0;
pub const GGRS_REQ_LOAD: i32 = 1;
pub const GGRS_REQ_ADVANCE: i32 = 2;

pub const GGRS_STATUS_CONFIRMED: u8 = 0;
pub const GGRS_STATUS_PREDICTED: u8 = 1;
pub const GGRS_STATUS_DISCONNECTED: u8 = 2;

pub const GGRS_PATH_PIPELINED: i32 = 0;
pub const GGRS_PATH_SEQUENTIAL: i32 = 1;
pub const GGRS_PATH_PIPELINED_CHAINS: i32 = 2;
pub const GGRS_PATH_PIPELINED_BATCHED: i32 = 3;

pub const GGRS_LANE_RUNNING: i32 = 0;
pub const GGRS_LANE_MISMATCH: i32 = 1;

pub const GGRS_TOK_SAVE: u32 = 0;
pub const GGRS_TOK_ADVANCE: u32 = 1;
pub const GGRS_TOK_LOAD: u32 = 2;
pub const GGRS_TOK_END: u32 = 3;
pub const GGRS_TOKENS_PER_WORD: i32 = 16;

pub const GGRS_BATCH_STATUS: i32 = 1;

pub const GGRS_BATCH_MAX_WORDS: i32 = 32;
pub const GGRS_BATCH_MAX_LOADS: i32 = 8;
pub const GGRS_BATCH_MAX_ADV: i32 = 128;
pub const GGRS_BATCH_MAX_SAVES: i32 = 256;

pub const GGRS_CODEC_OK: i32 = 0;
pub const GGRS_CODEC_E_BINCODE: i32 = -1;
pub const GGRS_CODEC_E_RLE: i32 = -2;
pub const GGRS_CODEC_E_DELTA: i32 = -3;
pub const GGRS_CODEC_E_CAP: i32 = -4;
pub const GGRS_CODEC_E_INVALID: i32 = -5;
pub const GGRS_CODEC_UNSUPPORTED: i32 = -6;
pub const GGRS_PACKET_NO_REFERENCE: i32 = -16;
pub const GGRS_PACKET_STOPPED: i32 = -17;
pub const GGRS_EMIT_CLOSED: i32 = -18;
pub const GGRS_EMIT_DISCONNECTED: i32 = -19;
pub const GGRS_EMIT_ROW_LOST: i32 = -20;
pub const GGRS_TIME_SYNC_KEEP: i32 = i32::MIN;
pub const GGRS_DESYNC_ROW_LOST: i32 = -21;
// endpoint poll: ggrs_p2p_poll_endpoints' net_events bits and ggrs_p2p_read_endpoint_state's state
pub const GGRS_NET_INTERRUPTED: i32 = 1;
pub const GGRS_NET_RESUMED: i32 = 2;
pub const GGRS_NET_DISCONNECTED: i32 = 4;
pub const GGRS_NET_SHUTDOWN: i32 = 8;
pub const GGRS_ENDPOINT_RUNNING: i32 = 0;
pub const GGRS_ENDPOINT_DISCONNECTED: i32 = 1;
pub const GGRS_ENDPOINT_SHUTDOWN: i32 = 2;
// wire envelope: message tags and ggrs_wire_unpack's slot_status codes (accepted: tag + 1, empty: 0)
pub const GGRS_WIRE_INPUT: i32 = 0;
pub const GGRS_WIRE_INPUT_ACK: i32 = 1;
pub const GGRS_WIRE_QUALITY_REPORT: i32 = 2;
pub const GGRS_WIRE_QUALITY_REPLY: i32 = 3;
pub const GGRS_WIRE_CHECKSUM_REPORT: i32 = 4;
pub const GGRS_WIRE_KEEP_ALIVE: i32 = 5;
pub const GGRS_WIRE_E_BINCODE: i32 = -22;
pub const GGRS_WIRE_E_SHAPE: i32 = -23;
pub const GGRS_WIRE_E_CAP: i32 = -24;
pub const GGRS_WIRE_E_CLOCK: i32 = -25;
pub const GGRS_WIRE_E_RANGE: i32 = -26;
// event queue: ggrs_event_record_t's kinds and ggrs_p2p_read_event_queue_state's status
pub const GGRS_EVENT_DISCONNECTED: i32 = 1;
pub const GGRS_EVENT_NETWORK_INTERRUPTED: i32 = 2;
pub const GGRS_EVENT_NETWORK_RESUMED: i32 = 3;
pub const GGRS_EVENT_WAIT_RECOMMENDATION: i32 = 4;
pub const GGRS_EVENT_DESYNC_DETECTED: i32 = 5;
pub const GGRS_EVENTS_LOST: i32 = -27;

/// One queued GgrsEvent (p2p_events.hip, spectator_events.hip): 16 bytes
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct ggrs_event_record_t {
    pub kind: u8,
    pub endpoint: u8,
    pub reserved: u16,
    pub call: i32,
    pub payload: u64,
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct ggrs_config_t {
    pub num_lanes: i32,
    pub num_players: i32,
    pub max_prediction: i32,
    pub check_distance: i32,
    pub input_delay: i32,
    pub input_capacity: i32,
    pub device: i32,
    pub trace_capacity: i32,
}

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct ggrs_request_t {
    pub kind: i32,
    pub frame: i32,
}

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct ggrs_lane_batch_t {
    pub token_words: i32,
    pub load_slots: i32,
    pub adv_rows: i32,
    pub save_rows: i32,
    pub tokens: *mut u32,
    pub load_frames: *mut i32,
    pub inputs: *mut u8,
    pub status: *mut u8,
    pub checksums: *mut u16,
    pub lane_result: *mut i32,
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct ggrs_branch_config_t {
    pub num_sessions: i32,
    pub num_players: i32,
    pub remote_mask: i32,
    pub window: i32,
    pub branches: i32,
    pub alphabet: i32,
    pub input_capacity: i32,
    pub device: i32,
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct ggrs_particle_config_t {
    pub num_sessions: i32,
    pub num_entities: i32,
    pub num_players: i32,
    pub max_prediction: i32,
    pub check_distance: i32,
    pub input_capacity: i32,
    pub device: i32,
    pub first_session_id: i32,
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct ggrs_p2p_config_t {
    pub num_sessions: i32,
    pub num_players: i32,
    pub local_mask: i32,
    pub input_delay: i32,
    pub max_prediction: i32,
    pub remote_latency: i32,
    pub predictor: i32,
    pub input_capacity: i32,
    pub trace_capacity: i32,
    pub device: i32,
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct ggrs_spectator_config_t {
    pub num_sessions: i32,
    pub num_players: i32,
    pub max_frames_behind: i32,
    pub catchup_speed: i32,
    pub input_capacity: i32,
    pub trace_capacity: i32,
    pub device: i32,
}

#[repr(C)]
pub struct ggrs_engine_t {
    _private: [u8; 0],
}

#[repr(C)]
pub struct ggrs_branch_engine_t {
    _private: [u8; 0],
}

#[repr(C)]
pub struct ggrs_particle_engine_t {
    _private: [u8; 0],
}

#[repr(C)]
pub struct ggrs_p2p_engine_t {
    _private: [u8; 0],
}

#[repr(C)]
pub struct ggrs_spectator_engine_t {
    _private: [u8; 0],
}

/// GGRS_SPECTATOR_NOTE: the host reports `player` disconnected with last frame `frame` (0 = no note).
pub const fn spectator_note(player: i32, frame: i32) -> i32 {
    1 | player << 1 | (frame + 1) << 3
}

extern "C" {
    pub fn ggrs_abi_version() -> i32;
    pub fn ggrs_last_error() -> *const c_char;

    // ---- the engine: SyncTest, lockstep and per-lane request lists
    pub fn ggrs_engine_create(cfg: *const ggrs_config_t, out: *mut *mut ggrs_engine_t) -> i32;
    pub fn ggrs_engine_destroy(eng: *mut ggrs_engine_t) -> i32;
    pub fn ggrs_engine_config(eng: *const ggrs_engine_t, out: *mut ggrs_config_t) -> i32;
    pub fn ggrs_add_local_inputs(eng: *mut ggrs_engine_t, first_frame: i32, n_frames: i32, inputs: *const u8) -> i32;
    pub fn ggrs_add_local_inputs_device(eng: *mut ggrs_engine_t, first_frame: i32, n_frames: i32,
                                        inputs_device: *const c_void) -> i32;
    pub fn ggrs_synctest_advance_frames(eng: *mut ggrs_engine_t, n_frames: i32) -> i32;
    pub fn ggrs_set_synctest_path(eng: *mut ggrs_engine_t, path: i32) -> i32;
    pub fn ggrs_handle_requests(eng: *mut ggrs_engine_t, reqs: *const ggrs_request_t, n_reqs: i32,
                                inputs: *const u8, status: *const u8) -> i32;
    pub fn ggrs_lane_batch_map(eng: *mut ggrs_engine_t, token_words: i32, load_slots: i32, adv_rows: i32,
                               save_rows: i32, out: *mut ggrs_lane_batch_t) -> i32;
    pub fn ggrs_lane_batch_run(eng: *mut ggrs_engine_t, batch: *const ggrs_lane_batch_t, flags: i32,
                               n_failed: *mut i32) -> i32;
    pub fn ggrs_handle_requests_lanes(eng: *mut ggrs_engine_t, reqs: *const ggrs_request_t, offsets: *const i32,
                                      inputs: *const u8, status: *const u8, save_checksums: *mut u16,
                                      lane_result: *mut i32) -> i32;
    pub fn ggrs_lane_batch_lds(eng: *mut ggrs_engine_t, token_words: i32, load_slots: i32, adv_rows: i32,
                               save_rows: i32, need_bytes: *mut i64, limit_bytes: *mut i64) -> i32;
    pub fn ggrs_lane_batch_submit(eng: *mut ggrs_engine_t, batch: *const ggrs_lane_batch_t, flags: i32) -> i32;
    pub fn ggrs_lane_batch_wait(eng: *mut ggrs_engine_t, n_failed: *mut i32) -> i32;
    pub fn ggrs_lane_encode(batch: *const ggrs_lane_batch_t, num_lanes: i64, num_players: i32, lane: i64,
                            reqs: *const ggrs_request_t, n_reqs: i32, inputs: *const u8, status: *const u8,
                            lane_frame: i32, bad_request: *mut i32) -> i32;
    pub fn ggrs_lane_shape(reqs: *const ggrs_request_t, n_reqs: i32, shape: *mut i32) -> i32;
    pub fn ggrs_lane_server(eng: *mut ggrs_engine_t, on: i32) -> i32;
    pub fn ggrs_read_lane_frames(eng: *mut ggrs_engine_t, frames: *mut i32) -> i32;
    pub fn ggrs_synchronize(eng: *mut ggrs_engine_t) -> i32;
    pub fn ggrs_current_frame(eng: *const ggrs_engine_t, out: *mut i32) -> i32;
    pub fn ggrs_read_mismatches(eng: *mut ggrs_engine_t, lane_status: *mut i32, mismatch_frame: *mut i32,
                                mismatch_mask: *mut u64) -> i32;
    pub fn ggrs_read_save_checksums(eng: *mut ggrs_engine_t, frame: i32, out: *mut u16) -> i32;
    pub fn ggrs_read_save_checksums_frames(eng: *mut ggrs_engine_t, frames: *const i32, n: i32, out: *mut u16) -> i32;
    pub fn ggrs_read_state(eng: *mut ggrs_engine_t, lane: i32, out: *mut u8) -> i32;
    pub fn ggrs_read_states(eng: *mut ggrs_engine_t, out: *mut u8) -> i32;
    pub fn ggrs_read_ring(eng: *mut ggrs_engine_t, lane: i32, frames: *mut i32, checksums: *mut u16,
                          states: *mut u8) -> i32;
    pub fn ggrs_read_trace(eng: *mut ggrs_engine_t, first_frame: i32, n_frames: i32, out: *mut u16) -> i32;
    pub fn ggrs_debug_corrupt_on_load(eng: *mut ggrs_engine_t, lane: i32, frame: i32) -> i32;
    pub fn ggrs_last_launch_ms(eng: *mut ggrs_engine_t, ms: *mut f32) -> i32;
    pub fn ggrs_timing_reset(eng: *mut ggrs_engine_t) -> i32;
    pub fn ggrs_timing_stop(eng: *mut ggrs_engine_t) -> i32;
    pub fn ggrs_timing_read(eng: *mut ggrs_engine_t, total_ms: *mut f32, launches: *mut i32) -> i32;

    // ---- speculative branch rollback (configs 3/4)
    pub fn ggrs_branch_engine_create(cfg: *const ggrs_branch_config_t, out: *mut *mut ggrs_branch_engine_t) -> i32;
    pub fn ggrs_branch_engine_destroy(eng: *mut ggrs_branch_engine_t) -> i32;
    pub fn ggrs_branch_engine_config(eng: *const ggrs_branch_engine_t, out: *mut ggrs_branch_config_t) -> i32;
    pub fn ggrs_branch_add_inputs(eng: *mut ggrs_branch_engine_t, first_frame: i32, n_frames: i32,
                                  inputs: *const u8) -> i32;
    pub fn ggrs_branch_speculate(eng: *mut ggrs_branch_engine_t) -> i32;
    pub fn ggrs_branch_confirm(eng: *mut ggrs_branch_engine_t, report_device: *mut c_void) -> i32;
    pub fn ggrs_branch_report_bytes(eng: *const ggrs_branch_engine_t, out: *mut i64) -> i32;
    pub fn ggrs_branch_synchronize(eng: *mut ggrs_branch_engine_t) -> i32;
    pub fn ggrs_branch_trunk_frame(eng: *const ggrs_branch_engine_t, out: *mut i32) -> i32;
    pub fn ggrs_branch_read_report(eng: *mut ggrs_branch_engine_t, checksums: *mut u16, survive_bits: *mut u64) -> i32;
    pub fn ggrs_branch_read_desync(eng: *mut ggrs_branch_engine_t, first_frame: *mut i32) -> i32;
    pub fn ggrs_branch_read_trunk(eng: *mut ggrs_branch_engine_t, session: i32, out: *mut u8) -> i32;
    pub fn ggrs_branch_read_lane(eng: *mut ggrs_branch_engine_t, lane: i64, frame: i32, checksum: *mut u16,
                                 out: *mut u8) -> i32;
    pub fn ggrs_branch_read_cells(eng: *mut ggrs_branch_engine_t, frame: i32, checksums: *mut u16, states: *mut u8)
                                  -> i32;
    pub fn ggrs_branch_timing_reset(eng: *mut ggrs_branch_engine_t) -> i32;
    pub fn ggrs_branch_timing_stop(eng: *mut ggrs_branch_engine_t) -> i32;
    pub fn ggrs_branch_timing_read(eng: *mut ggrs_branch_engine_t, total_ms: *mut f32, launches: *mut i32) -> i32;
    pub fn ggrs_branch_rounds(eng: *mut ggrs_branch_engine_t, n_rounds: i32) -> i32;
    pub fn ggrs_branch_set_round_launches(eng: *mut ggrs_branch_engine_t, on: i32) -> i32;
    pub fn ggrs_branch_set_stream(eng: *mut ggrs_branch_engine_t, stream: *mut c_void) -> i32;
    pub fn ggrs_branch_use_own_stream(eng: *mut ggrs_branch_engine_t) -> i32;
    pub fn ggrs_branch_round(eng: *mut ggrs_branch_engine_t, report_device: *mut c_void) -> i32;
    pub fn ggrs_branch_rounds_reports(eng: *mut ggrs_branch_engine_t, n_rounds: i32, reports_device: *mut c_void) -> i32;
    pub fn ggrs_branch_compare_peer_rows(eng: *mut ggrs_branch_engine_t, gathered: *const c_void, world: i32,
                                         rows_per_rank: i32, n_rows: i32, rank: i32, peer: i32, first_frame: i32,
                                         count_device: *mut i64, first_frame_device: *mut i64) -> i32;
    pub fn ggrs_branch_compare_peer(eng: *mut ggrs_branch_engine_t, gathered: *const c_void, world: i32, rank: i32,
                                    peer: i32, frame: i32, count_device: *mut i64,
                                    first_frame_device: *mut i64) -> i32;

    // ---- config-5 large-state stress game
    pub fn ggrs_particle_engine_create(cfg: *const ggrs_particle_config_t,
                                       out: *mut *mut ggrs_particle_engine_t) -> i32;
    pub fn ggrs_particle_engine_destroy(eng: *mut ggrs_particle_engine_t) -> i32;
    pub fn ggrs_particle_add_local_inputs(eng: *mut ggrs_particle_engine_t, first_frame: i32, n_frames: i32,
                                          inputs: *const u8) -> i32;
    pub fn ggrs_particle_synctest_advance_frames(eng: *mut ggrs_particle_engine_t, n_frames: i32) -> i32;
    pub fn ggrs_particle_synchronize(eng: *mut ggrs_particle_engine_t) -> i32;
    pub fn ggrs_particle_current_frame(eng: *const ggrs_particle_engine_t, out: *mut i32) -> i32;
    pub fn ggrs_particle_read_mismatches(eng: *mut ggrs_particle_engine_t, status: *mut i32, mismatch_frame: *mut i32,
                                         mismatch_mask: *mut u64) -> i32;
    pub fn ggrs_particle_read_state(eng: *mut ggrs_particle_engine_t, session: i32, out: *mut u8) -> i32;
    pub fn ggrs_particle_read_saved(eng: *mut ggrs_particle_engine_t, session: i32, frame: i32, checksum: *mut u16,
                                    out: *mut u8) -> i32;
    pub fn ggrs_particle_debug_corrupt_on_load(eng: *mut ggrs_particle_engine_t, session: i32, frame: i32) -> i32;
    pub fn ggrs_particle_timing_reset(eng: *mut ggrs_particle_engine_t) -> i32;
    pub fn ggrs_particle_timing_stop(eng: *mut ggrs_particle_engine_t) -> i32;
    pub fn ggrs_particle_timing_read(eng: *mut ggrs_particle_engine_t, total_ms: *mut f32, launches: *mut i32) -> i32;

    // ---- P2P sessions on the device
    pub fn ggrs_p2p_engine_create(cfg: *const ggrs_p2p_config_t, out: *mut *mut ggrs_p2p_engine_t) -> i32;
    pub fn ggrs_p2p_engine_destroy(eng: *mut ggrs_p2p_engine_t) -> i32;
    pub fn ggrs_p2p_engine_config(eng: *const ggrs_p2p_engine_t, out: *mut ggrs_p2p_config_t) -> i32;
    pub fn ggrs_p2p_add_inputs(eng: *mut ggrs_p2p_engine_t, first_frame: i32, n_frames: i32, inputs: *const u8) -> i32;
    pub fn ggrs_p2p_advance_frames(eng: *mut ggrs_p2p_engine_t, n_frames: i32) -> i32;
    pub fn ggrs_p2p_current_frame(eng: *const ggrs_p2p_engine_t, out: *mut i32) -> i32;
    pub fn ggrs_p2p_calls(eng: *const ggrs_p2p_engine_t, out: *mut i32) -> i32;
    pub fn ggrs_p2p_synchronize(eng: *mut ggrs_p2p_engine_t) -> i32;
    pub fn ggrs_p2p_read_state(eng: *mut ggrs_p2p_engine_t, session: i32, out: *mut u8) -> i32;
    pub fn ggrs_p2p_read_states(eng: *mut ggrs_p2p_engine_t, out: *mut u8) -> i32;
    pub fn ggrs_p2p_add_peer_reports(eng: *mut ggrs_p2p_engine_t, first_call: i32, n_calls: i32, reports: *const i32)
                                     -> i32;
    pub fn ggrs_p2p_read_ring(eng: *mut ggrs_p2p_engine_t, session: i32, frames: *mut i32, checksums: *mut u16,
                              states: *mut u8) -> i32;
    pub fn ggrs_p2p_read_stats(eng: *mut ggrs_p2p_engine_t, rollbacks: *mut i32, resim_frames: *mut i64) -> i32;
    pub fn ggrs_p2p_read_queues(eng: *mut ggrs_p2p_engine_t, out: *mut i32) -> i32;
    pub fn ggrs_p2p_read_trace(eng: *mut ggrs_p2p_engine_t, first_frame: i32, n: i32, out: *mut u16) -> i32;
    pub fn ggrs_p2p_timing_reset(eng: *mut ggrs_p2p_engine_t) -> i32;
    pub fn ggrs_p2p_timing_stop(eng: *mut ggrs_p2p_engine_t) -> i32;
    pub fn ggrs_p2p_timing_read(eng: *mut ggrs_p2p_engine_t, total_ms: *mut f32, launches: *mut i32) -> i32;
    pub fn ggrs_p2p_set_desync_detection(eng: *mut ggrs_p2p_engine_t, interval: i32) -> i32;
    pub fn ggrs_p2p_local_checksums(eng: *mut ggrs_p2p_engine_t, frame: i32, out: *mut u16, out_on_device: i32) -> i32;
    pub fn ggrs_p2p_compare_checksums(eng: *mut ggrs_p2p_engine_t, frame: i32, remote: *const u16,
                                      remote_on_device: i32, mask: *mut u64, n_differ: *mut i32) -> i32;
    pub fn ggrs_p2p_set_sparse_saving(eng: *mut ggrs_p2p_engine_t, on: i32) -> i32;
    pub fn ggrs_p2p_set_unstaged(eng: *mut ggrs_p2p_engine_t, form: i32) -> i32;
    pub fn ggrs_p2p_debug_desync(eng: *mut ggrs_p2p_engine_t, session: i32, frame: i32) -> i32;
    pub fn ggrs_p2p_set_arrival_schedule(eng: *mut ggrs_p2p_engine_t, on: i32) -> i32;
    pub fn ggrs_p2p_add_arrivals(
        eng: *mut ggrs_p2p_engine_t,
        first_call: i32,
        n_calls: i32,
        arrive_upto: *const i32,
        events: *const u8,
    ) -> i32;
    pub fn ggrs_p2p_read_sessions(
        eng: *mut ggrs_p2p_engine_t,
        frames: *mut i32,
        skipped: *mut i32,
        errors: *mut i32,
    ) -> i32;
    pub fn ggrs_p2p_read_reports(
        eng: *mut ggrs_p2p_engine_t,
        first_call: i32,
        n_calls: i32,
        frames: *mut i32,
        checksums: *mut u16,
        last_confirmed: *mut i32,
        local_last: *mut i32,
    ) -> i32;
    // packet feed (p2p_ingest.hip): the remote inputs as the wire packets each call received
    pub fn ggrs_p2p_set_packet_feed(eng: *mut ggrs_p2p_engine_t, max_packet_inputs: i32, packet_stride: i32) -> i32;
    pub fn ggrs_p2p_receive_packets(
        eng: *mut ggrs_p2p_engine_t,
        first_call: i32,
        n_calls: i32,
        start_frame: *const i32,
        packet_len: *const i32,
        packets: *const u8,
        events: *const u8,
        on_device: i32,
    ) -> i32;
    pub fn ggrs_p2p_read_packet_results(
        eng: *mut ggrs_p2p_engine_t,
        first_call: i32,
        n_calls: i32,
        status: *mut i32,
        ack_frame: *mut i32,
    ) -> i32;
    // packet emit (p2p_emit.hip): the sessions' outgoing Input message bodies, built on the device
    pub fn ggrs_p2p_set_packet_emit(eng: *mut ggrs_p2p_engine_t, max_pending_inputs: i32, out_stride: i32) -> i32;
    pub fn ggrs_p2p_emit_packets(
        eng: *mut ggrs_p2p_engine_t,
        first_call: i32,
        n_calls: i32,
        ack_in: *const i32,
        resend: *const u8,
        start_frame: *mut i32,
        packet_len: *mut i32,
        ack_frame: *mut i32,
        packets: *mut u8,
        on_device: i32,
    ) -> i32;
    pub fn ggrs_p2p_read_emit_state(
        eng: *mut ggrs_p2p_engine_t,
        last_acked: *mut i32,
        pending: *mut i32,
        status: *mut i32,
        closed_call: *mut i32,
    ) -> i32;
    // spectator emit (p2p_spec_emit.hip): the sessions' confirmed inputs to their spectators, built on the device
    pub fn ggrs_p2p_set_spectator_emit(
        eng: *mut ggrs_p2p_engine_t,
        num_spectators: i32,
        max_pending_inputs: i32,
        out_stride: i32,
    ) -> i32;
    pub fn ggrs_p2p_emit_spectator_packets(
        eng: *mut ggrs_p2p_engine_t,
        first_call: i32,
        n_calls: i32,
        ack_in: *const i32,
        resend: *const u8,
        start_frame: *mut i32,
        packet_len: *mut i32,
        notes: *mut i32,
        packets: *mut u8,
        on_device: i32,
    ) -> i32;
    pub fn ggrs_p2p_read_spectator_emit_state(
        eng: *mut ggrs_p2p_engine_t,
        next_spectator_frame: *mut i32,
        last_acked: *mut i32,
        pending: *mut i32,
        status: *mut i32,
        closed_call: *mut i32,
    ) -> i32;
    // time sync (p2p_time_sync.hip): frames_ahead and the wait recommendation per call, on the device
    pub fn ggrs_p2p_set_time_sync(eng: *mut ggrs_p2p_engine_t, fps: i32) -> i32;
    pub fn ggrs_p2p_time_sync(
        eng: *mut ggrs_p2p_engine_t,
        first_call: i32,
        n_calls: i32,
        rtt_ms: *const i32,
        remote_advantage: *const i32,
        local_advantage: *mut i32,
        frames_ahead: *mut i32,
        skip_frames: *mut i32,
        on_device: i32,
    ) -> i32;
    pub fn ggrs_p2p_read_time_sync_state(
        eng: *mut ggrs_p2p_engine_t,
        local_advantage: *mut i32,
        remote_advantage: *mut i32,
        rtt_ms: *mut i32,
        next_recommended_sleep: *mut i32,
        closed_call: *mut i32,
        windows: *mut i32,
    ) -> i32;
    // checksum comparison (p2p_desync.hip): on_checksum_report and DesyncDetected per call, on the device
    pub fn ggrs_p2p_set_desync_compare(eng: *mut ggrs_p2p_engine_t, max_events: i32) -> i32;
    pub fn ggrs_p2p_add_remote_reports(
        eng: *mut ggrs_p2p_engine_t,
        first_call: i32,
        n_calls: i32,
        frames: *const i32,
        checksums: *const u16,
        local_last: *const i32,
        on_device: i32,
    ) -> i32;
    pub fn ggrs_p2p_add_remote_reports_from(
        eng: *mut ggrs_p2p_engine_t,
        peer_eng: *mut ggrs_p2p_engine_t,
        first_call: i32,
        n_calls: i32,
    ) -> i32;
    pub fn ggrs_p2p_compare_reports(eng: *mut ggrs_p2p_engine_t, first_call: i32, n_calls: i32,
                                    n_events_total: *mut i32) -> i32;
    pub fn ggrs_p2p_read_desync_events(
        eng: *mut ggrs_p2p_engine_t,
        first: i32,
        max: i32,
        call: *mut i32,
        session: *mut i32,
        frame: *mut i32,
        local: *mut u16,
        remote: *mut u16,
        n_read: *mut i32,
    ) -> i32;
    pub fn ggrs_p2p_read_desync_state(
        eng: *mut ggrs_p2p_engine_t,
        status: *mut i32,
        n_events: *mut i32,
        first_call: *mut i32,
        first_frame: *mut i32,
        first_local: *mut i32,
        first_remote: *mut i32,
        refused: *mut i32,
        history: *mut i32,
        pending: *mut i32,
    ) -> i32;
    // endpoint poll (p2p_poll.hip): UdpProtocol::poll's timers and the disconnect timeout per call, on the device
    pub fn ggrs_p2p_set_endpoint_poll(
        eng: *mut ggrs_p2p_engine_t,
        disconnect_timeout_ms: u64,
        disconnect_notify_start_ms: u64,
        start_ms: u64,
    ) -> i32;
    pub fn ggrs_p2p_poll_endpoints(
        eng: *mut ggrs_p2p_engine_t,
        first_call: i32,
        n_calls: i32,
        now_ms: *const u64,
        kinds: *const u8,
        resend: *mut u8,
        send_ack: *mut u8,
        send_report: *mut u8,
        net_events: *mut u8,
        on_device: i32,
    ) -> i32;
    pub fn ggrs_p2p_read_endpoint_state(
        eng: *mut ggrs_p2p_engine_t,
        state: *mut i32,
        last_recv_ms: *mut u64,
        last_input_recv_ms: *mut u64,
        last_report_ms: *mut u64,
        shutdown_ms: *mut u64,
        flags: *mut i32,
        closed_call: *mut i32,
    ) -> i32;
    // spectator endpoint poll (p2p_spec_poll.hip): the same for the sessions' endpoints towards their spectators
    pub fn ggrs_p2p_set_spectator_poll(
        eng: *mut ggrs_p2p_engine_t,
        disconnect_timeout_ms: u64,
        disconnect_notify_start_ms: u64,
        start_ms: u64,
    ) -> i32;
    pub fn ggrs_p2p_poll_spectator_endpoints(
        eng: *mut ggrs_p2p_engine_t,
        first_call: i32,
        n_calls: i32,
        now_ms: *const u64,
        kinds: *const u8,
        close_in: *const u8,
        resend: *mut u8,
        send_report: *mut u8,
        net_events: *mut u8,
        on_device: i32,
    ) -> i32;
    pub fn ggrs_p2p_read_spectator_endpoint_state(
        eng: *mut ggrs_p2p_engine_t,
        state: *mut i32,
        last_recv_ms: *mut u64,
        last_input_recv_ms: *mut u64,
        last_report_ms: *mut u64,
        shutdown_ms: *mut u64,
        flags: *mut i32,
        closed_call: *mut i32,
    ) -> i32;
    // event queue (p2p_events.hip): every session's GgrsEvent queue on the device, drained in one call
    pub fn ggrs_p2p_set_event_queue(eng: *mut ggrs_p2p_engine_t, capacity: i32) -> i32;
    pub fn ggrs_p2p_collect_events(
        eng: *mut ggrs_p2p_engine_t,
        first_call: i32,
        n_calls: i32,
        events: *const u8,
        disc_req: *const u8,
        handled_inputs: *const u8,
        net_events: *const u8,
        spec_net_events: *const u8,
        skip_frames: *const i32,
        n_desync: i32,
        ds_call: *const i32,
        ds_session: *const i32,
        ds_frame: *const i32,
        ds_local: *const u16,
        ds_remote: *const u16,
        on_device: i32,
    ) -> i32;
    pub fn ggrs_p2p_drain_events(
        eng: *mut ggrs_p2p_engine_t,
        max_records: i32,
        session: *mut i32,
        records: *mut ggrs_event_record_t,
        n_read: *mut i32,
        n_left: *mut i32,
        on_device: i32,
    ) -> i32;
    pub fn ggrs_p2p_read_event_queue_state(
        eng: *mut ggrs_p2p_engine_t,
        length: *mut i32,
        dropped: *mut i32,
        status: *mut i32,
        closed_call: *mut i32,
        queue: *mut ggrs_event_record_t,
    ) -> i32;

    // ---- spectators (src/sessions/p2p_spectator_session.rs), batched
    pub fn ggrs_spectator_engine_create(cfg: *const ggrs_spectator_config_t, out: *mut *mut ggrs_spectator_engine_t) -> i32;
    pub fn ggrs_spectator_engine_destroy(eng: *mut ggrs_spectator_engine_t) -> i32;
    pub fn ggrs_spectator_engine_config(eng: *const ggrs_spectator_engine_t, out: *mut ggrs_spectator_config_t) -> i32;
    pub fn ggrs_spectator_add_inputs(eng: *mut ggrs_spectator_engine_t, first_frame: i32, n_frames: i32,
                                     inputs: *const u8) -> i32;
    pub fn ggrs_spectator_add_arrivals(eng: *mut ggrs_spectator_engine_t, first_call: i32, n_calls: i32,
                                       recv_upto: *const i32, notes: *const i32) -> i32;
    pub fn ggrs_spectator_advance_frames(eng: *mut ggrs_spectator_engine_t, n_calls: i32) -> i32;
    pub fn ggrs_spectator_calls(eng: *const ggrs_spectator_engine_t, out: *mut i32) -> i32;
    pub fn ggrs_spectator_synchronize(eng: *mut ggrs_spectator_engine_t) -> i32;
    pub fn ggrs_spectator_read_sessions(eng: *mut ggrs_spectator_engine_t, current_frame: *mut i32,
                                        last_recv: *mut i32, waited: *mut i32, errors: *mut i32) -> i32;
    pub fn ggrs_spectator_read_state(eng: *mut ggrs_spectator_engine_t, session: i32, out: *mut u8) -> i32;
    pub fn ggrs_spectator_read_states(eng: *mut ggrs_spectator_engine_t, out: *mut u8) -> i32;
    pub fn ggrs_spectator_read_trace(eng: *mut ggrs_spectator_engine_t, first_call: i32, n: i32, advanced: *mut u8,
                                     checksums: *mut u16) -> i32;
    pub fn ggrs_spectator_timing_reset(eng: *mut ggrs_spectator_engine_t) -> i32;
    pub fn ggrs_spectator_timing_stop(eng: *mut ggrs_spectator_engine_t) -> i32;
    pub fn ggrs_spectator_timing_read(eng: *mut ggrs_spectator_engine_t, total_ms: *mut f32, launches: *mut i32) -> i32;
    // the spectators' packet feed (UdpProtocol::on_input on the device, per-session input windows)
    pub fn ggrs_spectator_set_packet_feed(eng: *mut ggrs_spectator_engine_t, max_prediction: i32,
                                          max_packet_inputs: i32, packet_stride: i32) -> i32;
    pub fn ggrs_spectator_receive_packets(eng: *mut ggrs_spectator_engine_t, first_call: i32, n_calls: i32,
                                          start_frame: *const i32, packet_len: *const i32, packets: *const u8,
                                          notes: *const i32, on_device: i32) -> i32;
    pub fn ggrs_spectator_read_packet_results(eng: *mut ggrs_spectator_engine_t, first_call: i32, n_calls: i32,
                                              status: *mut i32, ack_frame: *mut i32) -> i32;
    // the spectators' endpoint poll (spectator_poll.hip): the host endpoint's timers and timeout per call
    pub fn ggrs_spectator_set_endpoint_poll(eng: *mut ggrs_spectator_engine_t, disconnect_timeout_ms: u64,
                                            disconnect_notify_start_ms: u64, start_ms: u64) -> i32;
    pub fn ggrs_spectator_poll_endpoints(eng: *mut ggrs_spectator_engine_t, first_call: i32, n_calls: i32,
                                         now_ms: *const u64, kinds: *const u8, events: *const u8, send_ack: *mut u8,
                                         send_report: *mut u8, net_events: *mut u8, on_device: i32) -> i32;
    pub fn ggrs_spectator_read_endpoint_state(eng: *mut ggrs_spectator_engine_t, last_recv_ms: *mut u64,
                                              last_input_recv_ms: *mut u64, last_report_ms: *mut u64, flags: *mut i32,
                                              disconnected_call: *mut i32) -> i32;
    // the spectators' event queue (spectator_events.hip)
    pub fn ggrs_spectator_set_event_queue(eng: *mut ggrs_spectator_engine_t, capacity: i32) -> i32;
    pub fn ggrs_spectator_collect_events(eng: *mut ggrs_spectator_engine_t, first_call: i32, n_calls: i32,
                                         handled_inputs: *const u8, net_events: *const u8, on_device: i32) -> i32;
    pub fn ggrs_spectator_drain_events(eng: *mut ggrs_spectator_engine_t, max_records: i32, session: *mut i32,
                                       records: *mut ggrs_event_record_t, n_read: *mut i32, n_left: *mut i32,
                                       on_device: i32) -> i32;
    pub fn ggrs_spectator_read_event_queue_state(eng: *mut ggrs_spectator_engine_t, length: *mut i32, dropped: *mut i32,
                                                 status: *mut i32, closed_call: *mut i32,
                                                 queue: *mut ggrs_event_record_t) -> i32;

    // ---- input wire codec, batched (src/network/compression.rs:14-182); device pointers
    pub fn ggrs_codec_encode(ref_: *const u8, pending: *const u8, count: *const i32, n_packets: i64,
                             input_bytes: i32, max_inputs: i32, out: *mut u8, out_stride: i32,
                             out_len: *mut i32, stream: *mut c_void) -> i32;
    pub fn ggrs_codec_decode(ref_: *const u8, packets: *const u8, packet_len: *const i32, n_packets: i64,
                             packet_stride: i32, input_bytes: i32, max_inputs: i32, out: *mut u8,
                             count: *mut i32, status: *mut i32, stream: *mut c_void) -> i32;
    pub fn ggrs_codec_encode_chunked(ref_: *const u8, pending: *const u8, count: *const i32, n_packets: i64,
                                     input_bytes: i32, max_inputs: i32, out: *mut u8, out_stride: i32,
                                     out_len: *mut i32, stream: *mut c_void) -> i32;
    pub fn ggrs_codec_decode_chunked(ref_: *const u8, packets: *const u8, packet_len: *const i32, n_packets: i64,
                                     packet_stride: i32, input_bytes: i32, max_inputs: i32, out: *mut u8,
                                     count: *mut i32, status: *mut i32, stream: *mut c_void) -> i32;
    pub fn ggrs_codec_max_packet_bytes(input_bytes: i32, max_inputs: i32) -> i32;
    pub fn ggrs_codec_set_direct(mode: i32) -> i32;

    // ---- wire envelope, batched (wire.hip): bincode Message datagrams <-> the units' arrays; device pointers
    pub fn ggrs_wire_max_datagram_bytes(num_statuses: i32, body_bytes: i32) -> i32;
    pub fn ggrs_wire_unpack(n_calls: i32, num_sessions: i32, slots: i32, num_statuses: i32, remote_mask: u32,
                            first_call: i32, dgrams: *const u8, dgram_stride: i32, dgram_len: *const i32,
                            now_ms: *const u64, packet_stride: i32, slot_status: *mut i32, start_frame: *mut i32,
                            packet_len: *mut i32, packets: *mut u8, ack_in: *mut i32, events: *mut u8,
                            disc_mask: *mut u8, last_frame: *mut i32, notes: *mut i32, remote_advantage: *mut i32,
                            ping: *mut u8, rtt_ms: *mut i32, report_frame: *mut i32, report_checksum: *mut u16,
                            kinds: *mut u8, stream: *mut c_void) -> i32;
    pub fn ggrs_wire_pack(n_calls: i32, num_sessions: i32, num_statuses: i32, magic: *const u16, now_ms: *const u64,
                          start_frame: *const i32, packet_len: *const i32, ack_frame: *const i32, packets: *const u8,
                          packet_stride: i32, disc_mask: *const u8, last_frame: *const i32,
                          disconnect_requested: *const u8, send_ack: *const u8, send_report: *const u8,
                          local_advantage: *const i32, kinds: *const u8, ping: *const u8, report_frame: *const i32,
                          report_checksum: *const u16, keep_alive: *const u8, dgrams: *mut u8, dgram_stride: i32,
                          dgram_len: *mut i32, stream: *mut c_void) -> i32;
}

/// The engine's last error message on this thread.
pub fn last_error() -> String {
    unsafe { std::ffi::CStr::from_ptr(ggrs_last_error()) }.to_string_lossy().into_owned()
}
