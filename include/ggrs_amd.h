/*
 * ggrs_amd.h -- C ABI of the MI355X batched rollback-resimulation engine.
 *
 * One engine owns L lanes.  A lane is one (session, branch): its own ex_game State, its own
 * saved-state ring and its own input stream.  Every call acts on all lanes at once: either one
 * request program for every lane (the fused SyncTest program, or a lockstep request list -- the
 * kinds and frames GGRS sessions in lockstep emit are identical, only inputs differ) or one list per
 * lane (ggrs_handle_requests_lanes / ggrs_lane_batch_run: P2P sessions that roll back to their own
 * frames).
 *
 * Replaces (caspark/ggrs 0.10.2, file:line):
 *   ggrs_engine_create         SessionBuilder::start_synctest_session (src/sessions/builder.rs:346-358)
 *                              + SyncLayer::new / SavedStates::new (src/sync_layer.rs:149-159,183-198)
 *                              + Game::new / State::new (examples/ex_game/ex_game.rs:67-76,246-269)
 *   ggrs_add_local_inputs      SyncTestSession::add_local_input (src/sessions/sync_test_session.rs:61-74)
 *                              feeding InputQueue::add_input (src/input_queue.rs:170-186) with the
 *                              session's input delay (src/input_queue.rs:233-265)
 *   ggrs_synctest_advance_frames
 *                              n x { SyncTestSession::advance_frame (sync_test_session.rs:85-150)
 *                              incl. checksums_consistent (:173-190) and adjust_gamestate (:192-217),
 *                              then Game::handle_requests (ex_game.rs:79-99) }
 *   ggrs_handle_requests       Game::handle_requests (ex_game.rs:79-99) for an ordered
 *                              Vec<GgrsRequest> (src/lib.rs:171-195): SaveGameState -> save_game_state
 *                              (ex_game.rs:103-108), LoadGameState -> load_game_state (:111-113),
 *                              AdvanceFrame -> advance_frame (:115-127)
 *   ggrs_read_save_checksums   the `Some(checksum)` a handler passes to GameStateCell::save
 *                              (sync_layer.rs:18-24), so a GGRS session can keep `data = None`
 *                              cells while the states live in HBM
 *   ggrs_read_mismatches       GgrsError::MismatchedChecksum { current_frame, mismatched_frames }
 *                              (src/error.rs:44-50), per lane
 *   ggrs_handle_requests_lanes Game::handle_requests for every lane's own Vec<GgrsRequest>, as
 *   ggrs_lane_batch_run        P2PSession::advance_frame emits them (p2p_session.rs:265-426)
 *
 * Errors: every function returns GGRS_OK (0) or a negative GGRS_E_* code; ggrs_last_error() gives
 * the message.  The reference panics (assert!) on precondition violations (sync_layer.rs:20,
 * 231-248; ex_game.rs:104); this ABI never unwinds and reports them as GGRS_E_PRECONDITION
 * without touching device state.  A checksum mismatch is data, not an error code.
 *
 * Threading: an engine is used by one host thread at a time; work is enqueued on the engine's
 * own HIP stream and the read functions synchronise with it.  No torch types cross this ABI.
 */
#ifndef GGRS_AMD_H
#define GGRS_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: GGRS_PATH_* renumbered (2, 3 = the pipelined forms), lane batches submitted and waited for
 * separately, host-side lane encoding, branch round forms
 * 3: ggrs_branch_set_stream(e, NULL) binds HIP's null stream (it used to select the engine's own
 * stream); ggrs_branch_use_own_stream returns to the engine's own
 * 4: P2P arrival schedules (ggrs_p2p_set_arrival_schedule, ggrs_p2p_add_arrivals,
 * ggrs_p2p_read_sessions)
 * 5: desync detection under arrival schedules (ggrs_p2p_read_reports)
 * 6: bulk reads for every-lane checks (ggrs_read_states, ggrs_p2p_read_states, ggrs_branch_read_cells);
 * lockstep mode under arrival schedules, peers' disconnect reports (ggrs_p2p_add_peer_reports);
 * added without a new version (nothing existing changed): the spectator engine and
 * GGRS_E_TOO_FAR_BEHIND; the P2P packet feed and packet emit; the spectators' packet feed; the P2P
 * engine's spectator emit (ggrs_p2p_set_spectator_emit) */
#define GGRS_ABI_VERSION 6

#define GGRS_OK 0
#define GGRS_E_INVALID (-1)      /* GgrsError::InvalidRequest: bad argument or configuration */
#define GGRS_E_PRECONDITION (-2) /* a reference assert! would have panicked */
#define GGRS_E_HIP (-3)          /* HIP runtime error (message from hipGetErrorString) */
#define GGRS_E_STATE (-4)        /* call not valid in the engine's current mode */
#define GGRS_E_TOO_FAR_BEHIND (-5) /* GgrsError::SpectatorTooFarBehind, per session (ggrs_spectator_read_sessions) */

#define GGRS_NULL_FRAME (-1) /* src/lib.rs:47 */

/* GgrsRequest kinds (src/lib.rs:171-195) */
#define GGRS_REQ_SAVE 0
#define GGRS_REQ_LOAD 1
#define GGRS_REQ_ADVANCE 2

/* InputStatus (src/lib.rs:106-113) as carried per player in the status bytes of an advance */
#define GGRS_STATUS_CONFIRMED 0
#define GGRS_STATUS_PREDICTED 1
#define GGRS_STATUS_DISCONNECTED 2

/* SyncTest execution paths (ggrs_set_synctest_path) */
#define GGRS_PATH_PIPELINED 0  /* default: concurrent rollback chains per session, one lane per
                                  (chain, player); picks CHAINS or BATCHED by wave packing */
#define GGRS_PATH_SEQUENTIAL 1 /* one lane per session, calls in order */
#define GGRS_PATH_PIPELINED_CHAINS 2  /* cd+1 chain lanes per player, when (cd+1) * padded players <= 64 */
#define GGRS_PATH_PIPELINED_BATCHED 3 /* check_distance 8: cd chain lanes per player, the chains'
                                         last advance batched every 8 frames (CHAINS otherwise) */

/* per-lane status */
#define GGRS_LANE_RUNNING 0
#define GGRS_LANE_MISMATCH 1 /* halted: SyncTestSession::advance_frame returned MismatchedChecksum */

typedef struct ggrs_config {
  int32_t num_lanes;      /* L >= 1: independent (session, branch) lanes */
  int32_t num_players;    /* 1..4 (ex_game.rs:70) */
  int32_t max_prediction; /* ring holds max_prediction + 1 saved states (sync_layer.rs:149-159) */
  int32_t check_distance; /* SyncTest check distance; must be < max_prediction (builder.rs:347) */
  int32_t input_delay;    /* local input delay in frames (builder.rs:154-158) */
  int32_t input_capacity; /* frames of queued input per lane; 0 = 128 (INPUT_QUEUE_LENGTH) */
  int32_t device;         /* HIP device ordinal */
  int32_t trace_capacity; /* frames of per-frame checksum trace kept on device; 0 = none */
} ggrs_config_t;

typedef struct ggrs_engine ggrs_engine_t;

typedef struct ggrs_request {
  int32_t kind;  /* GGRS_REQ_* */
  int32_t frame; /* Save/Load: the request's frame; Advance: ignored */
} ggrs_request_t;

int32_t ggrs_abi_version(void);
const char* ggrs_last_error(void);

int ggrs_engine_create(const ggrs_config_t* cfg, ggrs_engine_t** out);
int ggrs_engine_destroy(ggrs_engine_t* eng);
int ggrs_engine_config(const ggrs_engine_t* eng, ggrs_config_t* out);

/* Queue user inputs for frames [first_frame, first_frame + n_frames) of every lane.
 * inputs: [n_frames][num_lanes][num_players] bytes (Input.inp).  Frames must be added in order
 * starting at 0 (input_queue.rs:171-177); they enter the queue at frame + input_delay, frames
 * below the delay hold the default input (input_queue.rs:251-257).  `_device` takes a device
 * pointer (same layout) readable on the engine's stream. */
int ggrs_add_local_inputs(ggrs_engine_t* eng, int32_t first_frame, int32_t n_frames,
                          const uint8_t* inputs);
int ggrs_add_local_inputs_device(ggrs_engine_t* eng, int32_t first_frame, int32_t n_frames,
                                 const void* inputs_device);

/* Run n_frames SyncTest frames on every running lane (fused: one kernel launch; warm-up frames
 * f <= check_distance take one extra launch). */
int ggrs_synctest_advance_frames(ggrs_engine_t* eng, int32_t n_frames);
/* Choose the SyncTest kernel: GGRS_PATH_PIPELINED (default; a mismatch found there is re-run on
 * the sequential kernel from a checkpoint, so results are identical; sessions whose chains do not
 * fit one wavefront run sequentially), one of its two forms explicitly (_CHAINS, _BATCHED), or
 * GGRS_PATH_SEQUENTIAL. */
int ggrs_set_synctest_path(ggrs_engine_t* eng, int32_t path);

/* Execute an ordered request list on every lane (fused: one kernel launch).
 * inputs: [n_advance][num_lanes][num_players] Input.inp bytes, status: same shape InputStatus
 * bytes (NULL = all confirmed), one slice per AdvanceFrame in order.  Save checksums are kept on
 * device; read them with ggrs_read_save_checksums. */
int ggrs_handle_requests(ggrs_engine_t* eng, const ggrs_request_t* reqs, int32_t n_reqs,
                         const uint8_t* inputs, const uint8_t* status);

/* ---- Per-lane request lists: every lane is its own GGRS session.  A P2PSession rolls back to its
 * own first_incorrect frame and replays its own count of frames (p2p_session.rs:322-337,658-714),
 * so lanes' lists differ in kind, length and frames.  Two forms of one program:
 *   ggrs_handle_requests_lanes  the requests themselves, CSR over lanes: lane l's ordered
 *                               Vec<GgrsRequest> (src/lib.rs:171-195) is reqs[offsets[l] ..
 *                               offsets[l+1]); one checksum out per SaveGameState, in request order.
 *   ggrs_lane_batch_run         the same lists pre-encoded per lane (2-bit request kinds + the Load
 *                               frames: SURVEY.md 8b's rollback(load_frame, n, save_mask)) in
 *                               engine-owned pinned host memory the kernel reads directly, results
 *                               written straight back there: one launch, no copies.
 * Each lane's list is validated on the device before the lane's state is touched: a Load of a frame
 * its cell does not hold (SyncLayer::load_frame's assert, sync_layer.rs:248; ex_game.rs:112's
 * expect) or more requests of a kind than the batch holds fails the lane, which is left as it was
 * (the reference panics); every other lane runs.  ggrs_handle_requests_lanes also checks every
 * Save's frame against the lane's state frame (ex_game.rs:104).  Once an engine runs per-lane lists,
 * each lane keeps its own frame (ggrs_read_lane_frames, ggrs_read_ring); the lane-uniform calls
 * (ggrs_synctest_advance_frames, ggrs_handle_requests, ggrs_current_frame,
 * ggrs_read_save_checksums) return GGRS_E_STATE. */
#define GGRS_TOK_SAVE 0
#define GGRS_TOK_ADVANCE 1
#define GGRS_TOK_LOAD 2
#define GGRS_TOK_END 3
#define GGRS_TOKENS_PER_WORD 16

#define GGRS_BATCH_STATUS 1 /* ggrs_lane_batch_run reads the status rows (else every input Confirmed) */

/* shape limits of a lane batch */
#define GGRS_BATCH_MAX_WORDS 32 /* 512 requests per lane */
#define GGRS_BATCH_MAX_LOADS 8
#define GGRS_BATCH_MAX_ADV 128
#define GGRS_BATCH_MAX_SAVES 256

typedef struct ggrs_lane_batch {
  int32_t token_words;  /* W: words of request kinds per lane (16 per word) */
  int32_t load_slots;   /* LD: Load frames per lane (GGRS 0.10.2 emits at most 2 per list) */
  int32_t adv_rows;     /* A: AdvanceFrame rows per lane */
  int32_t save_rows;    /* S: SaveGameState checksums per lane */
  uint32_t* tokens;     /* [W][L]: lane l's request kinds in order, GGRS_TOK_* in 2 bits each,
                           least significant first, GGRS_TOK_END after the last (or W*16 long) */
  int32_t* load_frames; /* [LD][L]: frame of the lane's k-th LoadGameState */
  uint8_t* inputs;      /* [A][L][num_players]: Input.inp of the lane's a-th AdvanceFrame */
  uint8_t* status;      /* [A][L][num_players]: its InputStatus (GGRS_STATUS_*) */
  uint16_t* checksums;  /* out [S][L]: fletcher16 of the lane's k-th SaveGameState (the checksum a
                           handler passes to GameStateCell::save, sync_layer.rs:18-24) */
  int32_t* lane_result; /* out [L]: >= 0 the lane's frame after its list; < 0 -(1 + k) where k is
                           the index of the lane's first request that failed validation */
} ggrs_lane_batch_t;

/* Lay out (allocating or growing engine-owned pinned host memory) a batch of at least this shape
 * and return pointers into it; the pointers stay valid until the next _map with a larger shape or
 * ggrs_engine_destroy.  The caller fills tokens / load_frames / inputs (/ status) per call. */
int ggrs_lane_batch_map(ggrs_engine_t* eng, int32_t token_words, int32_t load_slots, int32_t adv_rows,
                        int32_t save_rows, ggrs_lane_batch_t* out);
/* Run every lane's list of a mapped batch (the counts in *batch may be lowered per call: rows past
 * them are not read).  flags: GGRS_BATCH_STATUS.  Returns when checksums and lane_result are in
 * host memory; GGRS_E_PRECONDITION when *n_failed lanes failed validation (the rest ran). */
int ggrs_lane_batch_run(ggrs_engine_t* eng, const ggrs_lane_batch_t* batch, int32_t flags, int32_t* n_failed);
/* LDS one lane block needs for a batch shape, and the device's limit per workgroup (bytes): shapes
 * with need > limit are GGRS_E_INVALID at ggrs_lane_batch_map. */
int ggrs_lane_batch_lds(ggrs_engine_t* eng, int32_t token_words, int32_t load_slots, int32_t adv_rows,
                        int32_t save_rows, int64_t* need_bytes, int64_t* limit_bytes);
/* ggrs_lane_batch_run in two halves.  _submit publishes the batch (to the lane server, or enqueues
 * one launch) and returns at once; _wait returns when its checksums and lane_result are in host
 * memory, with ggrs_lane_batch_run's result.  Between them the caller must not touch this batch's
 * memory, but may work on another engine's: a handler serving its sessions as two lane groups (two
 * engines) encodes and hands back one group while the other's batch is on the device.  Any other
 * call on the engine first waits for a submitted batch; its result is kept, and the next _wait
 * returns it (failed lanes included) instead of GGRS_E_STATE. */
int ggrs_lane_batch_submit(ggrs_engine_t* eng, const ggrs_lane_batch_t* batch, int32_t flags);
int ggrs_lane_batch_wait(ggrs_engine_t* eng, int32_t* n_failed);
/* Host-side encoding of one session's ordered request list (src/lib.rs:171-195) into column `lane`
 * of a lane batch -- the per-session work of a request handler, shared by every caller (the Rust
 * crate, the bench's C driver).  reqs[n_reqs]; inputs / status: [n_advance][num_players], one row
 * per AdvanceFrame in order (status NULL = Confirmed).  Writes every token word of the batch (END
 * after the list), the lane's Load frames and input / status rows.  lane_frame = the lane's frame
 * before the list (its previous lane_result; 0 for a fresh engine; GGRS_NULL_FRAME skips the check):
 * the batch carries no Save frames, so each SaveGameState's frame is checked here against the frame
 * the list has reached (Game::handle_requests' assert, ex_game.rs:104); on a mismatch the lane is
 * encoded with an empty list (it will not run), *bad_request = the request's index and the call
 * returns GGRS_E_PRECONDITION.  GGRS_E_INVALID: the list does not fit the batch's shape.  No device
 * access: usable without a GPU. */
int ggrs_lane_encode(const ggrs_lane_batch_t* batch, int64_t num_lanes, int32_t num_players, int64_t lane,
                     const ggrs_request_t* reqs, int32_t n_reqs, const uint8_t* inputs, const uint8_t* status,
                     int32_t lane_frame, int32_t* bad_request);
/* The batch shape one list needs: shape = {token words (ceil(n_reqs / 16): a list of exactly 16 W
 * requests needs no END token), Loads, AdvanceFrames, SaveGameStates}. */
int ggrs_lane_shape(const ggrs_request_t* reqs, int32_t n_reqs, int32_t* shape);
/* The generic form.  reqs: every lane's requests back to back, offsets: [num_lanes + 1]
 * (offsets[0] = 0).  inputs / status: [n_advance][num_players], one row per AdvanceFrame in the
 * same (lane, request) order; status NULL = all Confirmed.  save_checksums (may be NULL): one per
 * SaveGameState in the same order.  lane_result (may be NULL): [num_lanes] as in the batch.
 * GGRS_E_PRECONDITION when some lane's list failed validation (those lanes did not run). */
int ggrs_handle_requests_lanes(ggrs_engine_t* eng, const ggrs_request_t* reqs, const int32_t* offsets,
                               const uint8_t* inputs, const uint8_t* status, uint16_t* save_checksums,
                               int32_t* lane_result);
/* The lane server (default on): the first per-lane batch launches one persistent kernel that
 * serves every later batch -- the host publishes a batch by bumping an epoch in pinned host memory
 * and spins on per-block done flags, so a call costs one PCIe round trip instead of a launch plus a
 * stream synchronisation.  It ends (lanes' states back in device memory) before any other call
 * touches the engine's stream, when the host has been idle for 0.25 s, or by its own watchdog
 * after 1 s without a batch.  on = 0: one launch per batch.  At most GPU_MAX_HW_QUEUES (default 4)
 * servers run on one device at a time (each holds a hardware queue; a second server on the same
 * in-order queue would wait for the first to go idle): an engine that finds them all taken serves
 * its batches with one launch each until a server stops. */
int ggrs_lane_server(ggrs_engine_t* eng, int32_t on);
/* Every lane's current frame (its state's frame field): [num_lanes]. */
int ggrs_read_lane_frames(ggrs_engine_t* eng, int32_t* frames);

/* Block until all work queued on the engine's stream has finished. */
int ggrs_synchronize(ggrs_engine_t* eng);
/* Frame the engine's session is at (SyncTestSession::current_frame, sync_test_session.rs:153). */
int ggrs_current_frame(const ggrs_engine_t* eng, int32_t* out);
/* Per-lane status / mismatch: each array has num_lanes entries (any may be NULL).  mask bit k
 * set <=> frame (mismatch_frame - check_distance + k) mismatched. */
int ggrs_read_mismatches(ggrs_engine_t* eng, int32_t* lane_status, int32_t* mismatch_frame,
                         uint64_t* mismatch_mask);
/* Checksum stored with the saved cell of `frame` for every lane (num_lanes u16). */
int ggrs_read_save_checksums(ggrs_engine_t* eng, int32_t frame, uint16_t* out);
/* The same for n frames in one device-to-host transfer wait: out [n][num_lanes] (a request list's
 * saves, read once after ggrs_handle_requests instead of one synchronisation per save). */
int ggrs_read_save_checksums_frames(ggrs_engine_t* eng, const int32_t* frames, int32_t n, uint16_t* out);
/* Current game state of one lane as bincode bytes (36 + 20 * num_players). */
int ggrs_read_state(ggrs_engine_t* eng, int32_t lane, uint8_t* out);
/* ggrs_read_state for every lane, one transfer: out[num_lanes][36 + 20 * num_players]. */
int ggrs_read_states(ggrs_engine_t* eng, uint8_t* out);
/* Saved-state ring of one lane: frames[R], checksums[R], states[R][36 + 20 * num_players]. */
int ggrs_read_ring(ggrs_engine_t* eng, int32_t lane, int32_t* frames, uint16_t* checksums,
                   uint8_t* states);
/* Per-frame display checksum trace (fletcher16 of the state after each frame's final
 * AdvanceFrame, ex_game.rs:121-126) for frames [first_frame, first_frame + n_frames):
 * out[n_frames][num_lanes].  Requires trace_capacity > 0 and frames still held. */
int ggrs_read_trace(ggrs_engine_t* eng, int32_t first_frame, int32_t n_frames, uint16_t* out);

/* Fault injection (tests): after the LoadGameState of SyncTest call `frame`, flip the lowest
 * bit of player 0's x on `lane` -- a non-deterministic simulation the SyncTest must catch. */
int ggrs_debug_corrupt_on_load(ggrs_engine_t* eng, int32_t lane, int32_t frame);

/* Average device time per fused launch of the last timed span (ggrs_timing_reset .. _read), ms. */
int ggrs_last_launch_ms(ggrs_engine_t* eng, float* ms);
/* Time the fused launches from now on: one HIP event pair on the engine's stream brackets the
 * whole span (no per-launch events); _read synchronises, returns the span's milliseconds (launch
 * gaps included) and the number of fused launches in it, and stops collecting. */
int ggrs_timing_reset(ggrs_engine_t* eng);
/* Close the span without waiting: records its end event right behind the last launch (a caller
 * that then synchronises the stream itself reads the same span without an extra host round trip
 * inside its own wall clock).  _read after _stop reports that span.  Exception: a running lane
 * server is stopped first (the event would otherwise queue behind the persistent kernel), which
 * waits for a submitted batch and for the server to leave its loop. */
int ggrs_timing_stop(ggrs_engine_t* eng);
int ggrs_timing_read(ggrs_engine_t* eng, float* total_ms, int32_t* launches);

/* ---------------------------------------------------------------------------------------------
 * Speculative branch rollback (P2P).  Lane = (session, branch), lane = session * branches + branch.
 * A round = ggrs_branch_speculate (every lane: LoadGameState(trunk frame) of its session, then
 * window x (AdvanceFrame, SaveGameState) -- P2PSession::adjust_gamestate, p2p_session.rs:658-714,
 * plus the save of the current frame, :337 -- with the remote players' inputs from the branch
 * generator that replaces InputQueue prediction, input_queue.rs:104-167) followed by
 * ggrs_branch_confirm (the remote inputs of the trunk frame arrive: the trunk replays that frame
 * with them, every lane learns whether its branch survived -- assumed exactly those inputs,
 * input_queue.rs:199-218 -- and the per-session checksum + survival bits form the report that
 * multi-GPU runs all-gather, the ChecksumReport exchange of p2p_session.rs:939-975).
 */
typedef struct ggrs_branch_config {
  int32_t num_sessions;   /* S >= 1 */
  int32_t num_players;    /* 1..4 */
  int32_t remote_mask;    /* bit p: player p is remote (inputs confirmed late); others local */
  int32_t window;         /* W: frames speculated per round (1..62); ring = W + 1 saved states */
  int32_t branches;       /* B per session: 1 = PredictRepeatLast (lib.rs:390-395); A^E =
                             enumerate the first remote player over E frames, then hold */
  int32_t alphabet;       /* A: remote input values enumerated (16 for ex_game's 4 buttons) */
  int32_t input_capacity; /* frames of queued inputs per session; 0 = 128 */
  int32_t device;
} ggrs_branch_config_t;

typedef struct ggrs_branch_engine ggrs_branch_engine_t;

int ggrs_branch_engine_create(const ggrs_branch_config_t* cfg, ggrs_branch_engine_t** out);
int ggrs_branch_engine_destroy(ggrs_branch_engine_t* eng);
int ggrs_branch_engine_config(const ggrs_branch_engine_t* eng, ggrs_branch_config_t* out);
/* True inputs of every player for frames [first_frame, first_frame + n_frames):
 * [n_frames][num_sessions][num_players].  Remote players' values are only read once the frame
 * is confirmed (and as the repeat-last prediction source for later frames). */
int ggrs_branch_add_inputs(ggrs_branch_engine_t* eng, int32_t first_frame, int32_t n_frames,
                           const uint8_t* inputs);
int ggrs_branch_speculate(ggrs_branch_engine_t* eng);
/* Confirm the trunk frame; if report_device != NULL the round's report is also copied there
 * (device pointer, ggrs_branch_report_bytes bytes: [S] u16 checksums, padded to 8 bytes, then
 * ceil(L/64) u64 survival words) on the engine's stream. */
int ggrs_branch_confirm(ggrs_branch_engine_t* eng, void* report_device);
int ggrs_branch_report_bytes(const ggrs_branch_engine_t* eng, int64_t* out);
int ggrs_branch_synchronize(ggrs_branch_engine_t* eng);
int ggrs_branch_trunk_frame(const ggrs_branch_engine_t* eng, int32_t* out);
int ggrs_branch_read_report(ggrs_branch_engine_t* eng, uint16_t* checksums, uint64_t* survive_bits);
/* per session: first trunk frame at which a surviving branch's saved state disagreed with the
 * replayed trunk (a desync), or -1 */
int ggrs_branch_read_desync(ggrs_branch_engine_t* eng, int32_t* first_frame);
int ggrs_branch_read_trunk(ggrs_branch_engine_t* eng, int32_t session, uint8_t* out);
/* the saved state (bincode) and checksum of `frame` in one lane's ring (after prefix-shared rounds:
 * the cell of the lane's prefix representative, which holds the same state) */
int ggrs_branch_read_lane(ggrs_branch_engine_t* eng, int64_t lane, int32_t frame, uint16_t* checksum,
                          uint8_t* out);
/* ggrs_branch_read_lane for every lane at once (checking every lane against a CPU replay):
 * checksums [num_sessions * branches], states [num_sessions * branches][36 + 20 P] or NULL */
int ggrs_branch_read_cells(ggrs_branch_engine_t* eng, int32_t frame, uint16_t* checksums, uint8_t* states);
int ggrs_branch_timing_reset(ggrs_branch_engine_t* eng);
int ggrs_branch_timing_stop(ggrs_branch_engine_t* eng); /* as ggrs_timing_stop */
int ggrs_branch_timing_read(ggrs_branch_engine_t* eng, float* total_ms, int32_t* launches);
/* n_rounds x (ggrs_branch_speculate, ggrs_branch_confirm without a report copy) issued back to
 * back from native code; while timing is collected one event pair brackets the whole batch */
int ggrs_branch_rounds(ggrs_branch_engine_t* eng, int32_t n_rounds);
/* rounds() as one launch (on = 0, default: every block replays the trunks of its own sessions, so
 * no launch boundary is needed between rounds; when the enumerated player is the only remote one the
 * launch is prefix-shared -- each lane advances only that player, the local players' frames are
 * computed once per block and session, and a cell at depth k is saved once per distinct k+1-digit
 * prefix, by branch b mod A^min(k+1, E); ggrs_branch_read_lane resolves a lane's cell to it), as
 * 2 n launches of speculate / confirm (on = 1), or as one launch without prefix sharing (on = 2) */
int ggrs_branch_set_round_launches(ggrs_branch_engine_t* eng, int32_t on);
/* Enqueue every launch and copy from now on on `stream` (a hipStream_t; NULL = HIP's null stream,
 * as torch.cuda.current_stream() reports its default stream -- ABI 3; before it NULL meant the
 * engine's own non-blocking stream, which does not order with the null stream),
 * e.g. the stream a collective library orders its all-gather after: speculate, confirm (with its
 * report copy) and the report exchange then follow each other on the device with no host
 * synchronisation (multi-GPU configs 3/4, ggrs_amd/exchange.py ReportExchange).  Work queued
 * before the switch is ordered before work queued after it. */
int ggrs_branch_set_stream(ggrs_branch_engine_t* eng, void* stream);
/* Back to the engine's own (non-blocking) stream, the one it was created with; work queued before
 * the switch is ordered before work queued after it. */
int ggrs_branch_use_own_stream(ggrs_branch_engine_t* eng);
/* One round (speculate + confirm) as one launch; the round's report is also written to
 * report_device (device pointer, same layout as ggrs_branch_confirm's copy; NULL = none) by the
 * kernel itself -- the per-round call of the multi-GPU exchange loop. */
int ggrs_branch_round(ggrs_branch_engine_t* eng, void* report_device);
/* n rounds as one launch (ggrs_branch_rounds) with every round's report also written by the
 * kernel into row r of reports_device ([n][report_bytes], device) -- a batch of the multi-GPU
 * exchange loop, all-gathered once. */
int ggrs_branch_rounds_reports(ggrs_branch_engine_t* eng, int32_t n_rounds, void* reports_device);
/* Desync detection between peer replicas (compare_local_checksums_against_peers,
 * p2p_session.rs:904-937): `gathered` = world all-gathered reports ([world][report_bytes], device);
 * sessions whose checksum differs between rows `rank` and `peer` are added to *count_device
 * (device int64), and *first_frame_device (device int64, initialise to -1) takes `frame` if it is
 * still -1 and any differ.  Enqueued on the engine's stream, no host synchronisation. */
int ggrs_branch_compare_peer(ggrs_branch_engine_t* eng, const void* gathered, int32_t world, int32_t rank,
                             int32_t peer, int32_t frame, int64_t* count_device, int64_t* first_frame_device);
/* The same over a batch of rounds gathered at once: `gathered` = [world][rows_per_rank][report_bytes]
 * (each rank's reports of rows_per_rank consecutive rounds, one all-gather per batch), rows 0 ..
 * n_rows-1 compared, row k standing for frame first_frame + k; one launch. */
int ggrs_branch_compare_peer_rows(ggrs_branch_engine_t* eng, const void* gathered, int32_t world,
                                  int32_t rows_per_rank, int32_t n_rows, int32_t rank, int32_t peer,
                                  int32_t first_frame, int64_t* count_device, int64_t* first_frame_device);

/* ---------------------------------------------------------------------------------------------
 * Config-5 large-state stress game (defined by this build; ggrs_amd/csrc/particles.h):
 * a session is one frame counter + num_entities x 100-byte entities (an ex_game ship + 80 bytes
 * of integer payload), ~1 MB at 10k entities, so every Load/Save of the SyncTest program
 * (sync_test_session.rs:85-150) is an HBM stream.  One engine = num_sessions sessions.
 */
typedef struct ggrs_particle_config {
  int32_t num_sessions;
  int32_t num_entities;     /* multiple of 4, <= 160000 */
  int32_t num_players;      /* input bytes per frame; entity e plays player e % num_players */
  int32_t max_prediction;   /* ring = max_prediction + 1 states per session */
  int32_t check_distance;   /* 0..62, < max_prediction */
  int32_t input_capacity;   /* frames of queued input; 0 = 128 */
  int32_t device;
  int32_t first_session_id; /* global id of session 0 (seeds the initial payload) */
} ggrs_particle_config_t;

typedef struct ggrs_particle_engine ggrs_particle_engine_t;

int ggrs_particle_engine_create(const ggrs_particle_config_t* cfg, ggrs_particle_engine_t** out);
int ggrs_particle_engine_destroy(ggrs_particle_engine_t* eng);
/* inputs [n_frames][num_sessions][num_players], frames added in order from 0 (no input delay) */
int ggrs_particle_add_local_inputs(ggrs_particle_engine_t* eng, int32_t first_frame, int32_t n_frames,
                                   const uint8_t* inputs);
int ggrs_particle_synctest_advance_frames(ggrs_particle_engine_t* eng, int32_t n_frames);
int ggrs_particle_synchronize(ggrs_particle_engine_t* eng);
int ggrs_particle_current_frame(const ggrs_particle_engine_t* eng, int32_t* out);
int ggrs_particle_read_mismatches(ggrs_particle_engine_t* eng, int32_t* status, int32_t* mismatch_frame,
                                  uint64_t* mismatch_mask);
/* current state of one session in the declared layout (4 + 100 * num_entities bytes) */
int ggrs_particle_read_state(ggrs_particle_engine_t* eng, int32_t session, uint8_t* out);
/* the saved cell of `frame` (checksum and/or declared-layout bytes) */
int ggrs_particle_read_saved(ggrs_particle_engine_t* eng, int32_t session, int32_t frame, uint16_t* checksum,
                             uint8_t* out);
int ggrs_particle_debug_corrupt_on_load(ggrs_particle_engine_t* eng, int32_t session, int32_t frame);
int ggrs_particle_timing_reset(ggrs_particle_engine_t* eng);
int ggrs_particle_timing_stop(ggrs_particle_engine_t* eng); /* as ggrs_timing_stop */
int ggrs_particle_timing_read(ggrs_particle_engine_t* eng, float* total_ms, int32_t* launches);

/* ---------------------------------------------------------------------------------------------
 * P2P rollback decision: num_sessions independent P2PSessions of one peer,
 * each call = P2PSession::advance_frame (src/sessions/p2p_session.rs:265-426) + the ex_game
 * handler, with every remote player's InputQueue prediction (src/input_queue.rs:104-230) on the
 * device.  Rollback mode, sparse saving off, every player connected.  Network model: the remote
 * players' input of frame g arrives at the start of call g + remote_latency (poll_remote_clients
 * :430-446 -> handle_event Event::Input :880-895 -> SyncLayer::add_remote_input,
 * src/sync_layer.rs:271-277); the remote peer runs with input delay 0.
 */
typedef struct ggrs_p2p_config {
  int32_t num_sessions;
  int32_t num_players;     /* 1..4 (ex_game.rs:70) */
  int32_t local_mask;      /* bit p: player p is local to this peer; at least one player is remote */
  int32_t input_delay;     /* local players' frame delay (SessionBuilder::with_input_delay, builder.rs:150) */
  int32_t max_prediction;  /* builder.rs with_max_prediction_window; ring = max_prediction + 1; 0 =
                              lockstep mode (builder.rs:134-147): a call advances only once the
                              current frame's inputs are confirmed from every player, and never
                              saves, loads or resimulates (p2p_session.rs:301-310,393-407) */
  int32_t remote_latency;  /* 1 .. max_prediction-1 frames (any >= 1 in lockstep mode) */
  int32_t predictor;       /* 0 PredictRepeatLast, 1 PredictDefault (src/lib.rs:390-406) */
  int32_t input_capacity;  /* frames of queued input rows; 0 = 256 */
  int32_t trace_capacity;  /* calls of display checksums kept (0: none) */
  int32_t device;
} ggrs_p2p_config_t;

typedef struct ggrs_p2p_engine ggrs_p2p_engine_t;

int ggrs_p2p_engine_create(const ggrs_p2p_config_t* cfg, ggrs_p2p_engine_t** out);
int ggrs_p2p_engine_destroy(ggrs_p2p_engine_t* eng);
int ggrs_p2p_engine_config(const ggrs_p2p_engine_t* eng, ggrs_p2p_config_t* out);
/* inputs [n_frames][num_sessions][num_players]: row g holds the local players' add_local_input
 * (p2p_session.rs:219-246) of call g and the remote players' input of frame g (what the remote
 * peer sends, src/network/protocol.rs:564-642); rows are added in order from 0 */
int ggrs_p2p_add_inputs(ggrs_p2p_engine_t* eng, int32_t first_frame, int32_t n_frames, const uint8_t* inputs);
/* n_frames calls of advance_frame for every session; InvalidRequest when a call's row is missing */
int ggrs_p2p_advance_frames(ggrs_p2p_engine_t* eng, int32_t n_frames);
/* P2PSession::current_frame (p2p_session.rs:555-558); ggrs_p2p_calls: advance_frame calls made (the
 * same in rollback mode, where every call advances) */
int ggrs_p2p_current_frame(const ggrs_p2p_engine_t* eng, int32_t* out);
int ggrs_p2p_calls(const ggrs_p2p_engine_t* eng, int32_t* out);
int ggrs_p2p_synchronize(ggrs_p2p_engine_t* eng);
int ggrs_p2p_read_state(ggrs_p2p_engine_t* eng, int32_t session, uint8_t* out);
/* ggrs_p2p_read_state for every session, one transfer: out[num_sessions][36 + 20 * num_players] */
int ggrs_p2p_read_states(ggrs_p2p_engine_t* eng, uint8_t* out);
/* the session's saved-state ring (SavedStates, sync_layer.rs:144-166): per slot frame, checksum,
 * bincode state (36 + 20 P bytes) */
int ggrs_p2p_read_ring(ggrs_p2p_engine_t* eng, int32_t session, int32_t* frames, uint16_t* checksums,
                       uint8_t* states);
/* per session: number of rollbacks (adjust_gamestate calls) and resimulated frames so far */
int ggrs_p2p_read_stats(ggrs_p2p_engine_t* eng, int32_t* rollbacks, int64_t* resim_frames);
/* every session's InputQueue prediction state, [4][num_players][num_sessions] i32: prediction.frame,
 * prediction.input, first_incorrect_frame, last_requested_frame (input_queue.rs:10-37) */
int ggrs_p2p_read_queues(ggrs_p2p_engine_t* eng, int32_t* out);
/* [n][num_sessions] fletcher16 of each session's state after the final AdvanceFrame of calls
 * first_frame .. first_frame+n-1 (ex_game.rs:121-126) */
int ggrs_p2p_read_trace(ggrs_p2p_engine_t* eng, int32_t first_frame, int32_t n, uint16_t* out);
int ggrs_p2p_timing_reset(ggrs_p2p_engine_t* eng);
int ggrs_p2p_timing_stop(ggrs_p2p_engine_t* eng); /* as ggrs_timing_stop */
int ggrs_p2p_timing_read(ggrs_p2p_engine_t* eng, float* total_ms, int32_t* launches);

/* ---- P2P desync detection (SessionBuilder::with_desync_detection_mode, builder.rs:197-203;
 * DesyncDetection::On { interval }, src/lib.rs:71-80).  Replaces P2PSession's
 * check_checksum_send_interval (p2p_session.rs:939-975) for every session at once: at call
 * frame_to_send + remote_latency + 1 (when last_confirmed_frame and last_saved_frame reach it) the
 * saved cell's checksum of frame_to_send = interval, 2 interval, ... enters a device-resident
 * local_checksum_history of MAX_CHECKSUM_HISTORY_SIZE = 32 reports (protocol.rs:27).  The host
 * exchanges reports between peers (UdpProtocol::send_checksum_report, protocol.rs:692-698) and
 * compares received ones (compare_local_checksums_against_peers, p2p_session.rs:904-937) with
 * ggrs_p2p_compare_checksums; ggrs_amd/desync.py holds the pending-report bookkeeping. */
/* interval 0 = Off.  Part of the session's configuration: only before the first call. */
int ggrs_p2p_set_desync_detection(ggrs_p2p_engine_t* eng, int32_t interval);
/* [num_sessions] u16: the local checksum report of `frame` (host or device destination);
 * GGRS_E_PRECONDITION when `frame` is not a report frame sent so far or left the history */
int ggrs_p2p_local_checksums(ggrs_p2p_engine_t* eng, int32_t frame, uint16_t* out, int32_t out_on_device);
/* compare the local report of `frame` with a peer's [num_sessions] report: bit s of mask
 * (ceil(num_sessions/64) u64, host) set where they differ -- a GgrsEvent::DesyncDetected
 * (src/lib.rs:158-167) for session s; *n_differ = number of such sessions */
int ggrs_p2p_compare_checksums(ggrs_p2p_engine_t* eng, int32_t frame, const uint16_t* remote,
                               int32_t remote_on_device, uint64_t* mask, int32_t* n_differ);
/* Sparse saving (SessionBuilder::with_sparse_saving_mode, builder.rs:160-169): rollbacks load the
 * last saved state and save only min_confirmed (adjust_gamestate, p2p_session.rs:666-702), the
 * current frame is saved only when the last save would leave the prediction window
 * (check_last_saved_state :819-843), last_confirmed_frame never passes the last save
 * (sync_layer.rs:323-326).  Part of the configuration: only before the first call. */
int ggrs_p2p_set_sparse_saving(ggrs_p2p_engine_t* eng, int32_t on);
/* kernel form (comparison and tests): 0 = default (each session's calls flattened into its own
 * step sequence, input rows staged in LDS, with or without sparse saving), 1 = calls in
 * lockstep with input rows read from global memory, 2 = calls in lockstep with staged rows,
 * 3 = the flattened form with the session rings in HBM (the default keeps a block's rings in LDS
 * for the launch when they fit beside the other blocks on the CU, else it runs this form),
 * 4 = chains: every call as the chain of remote_latency + 1 advances from the confirmed state that
 * the fixed-latency network makes it (LoadGameState(f - D), D frames replayed, the call's own
 * advance), (D + 1) x players lanes per session, for engines whose sessions would fill at most one
 * wave per CU in the flattened form (the default picks it there); plain launches only -- no desync
 * detection, trace, debug flip or sparse saving (GGRS_E_STATE when forced otherwise); the first D
 * calls run on the flattened form.  Same states, rings, statistics and queues as every other form.
 * 5 = the flattened form with LDS rings, stepping every remote InputQueue's bookkeeping per frame;
 * 6 = canonical flattened form (the default for plain launches that do not take the chains form):
 * the rollback decision of call f is the remote input of frame f - D against the prediction made
 * from frame f - D - 1, the replay's remote inputs the confirmed and then the predicted ones -- the
 * queue state the fixed-latency network implies, written back at the end; with sparse saving on
 * (no trace or debug flip) the same form replays from the last save and saves min_confirmed. */
int ggrs_p2p_set_unstaged(ggrs_p2p_engine_t* eng, int32_t form);
/* test hook: the AdvanceFrame from `frame` of `session` flips the lowest bit of player 0's x on
 * every (re)simulation -- a deterministic desync of this peer (session -1: off) */
int ggrs_p2p_debug_desync(ggrs_p2p_engine_t* eng, int32_t session, int32_t frame);

/* ---- Arrival schedules: the network of a real match, per session.
 * Replaces the fixed remote_latency model by each session's own remote-arrival table, so every
 * session rolls back to its own earliest misprediction (InputQueue::add_input_by_frame's
 * first_incorrect_frame, src/input_queue.rs:190-230 -> check_simulation_consistency,
 * src/sync_layer.rs:343-353) with its own depth, a call at the prediction threshold saves but does
 * not advance (frames_ahead >= max_prediction, p2p_session.rs:393-423), and a disconnected remote
 * player (handle_event Event::Disconnected :866-878 -> disconnect_player_at_frame :618-655) rolls
 * the session back to its last frame + 1 and is replayed with InputStatus::Disconnected (ex_game
 * input 4, src/sync_layer.rs:280-293).  Call c: (1) the remote frames (delivered, arrive_upto[c]]
 * arrive, in order, for every remote player not disconnected; (2) Event::Disconnected for each
 * remote player k with bit k of events[c] (ascending k); (3) add_local_input of every local player
 * with input row c's byte, for the session's current frame (a call that did not advance repeats its
 * frame, and InputQueue::add_input drops the repeat, input_queue.rs:170-186); (4) advance_frame.
 * Input row g (ggrs_p2p_add_inputs) = the local players' input of call g and the remote players'
 * input of frame g, as in the fixed-latency model.  max_prediction 0 is lockstep mode (no saves,
 * no rollbacks, a call advances only when last_confirmed_frame == current_frame, :301-304,
 * 393-397); sparse saving allowed in rollback mode; the display trace per call (trace_capacity > 0: the
 * checksum after the call's last AdvanceFrame, ggrs_p2p_read_trace indexed by call); peers' disconnect reports
 * (ggrs_p2p_add_peer_reports) after (2); desync detection (ggrs_p2p_set_desync_detection, without sparse
 * saving) per session: ggrs_p2p_read_reports; remote_latency is ignored.  A session whose
 * call would make the reference panic (a remote input no longer in the input rows, or one that a
 * remote InputQueue's 128 entries have no room for -- a frame at or past max(last_confirmed_frame, 1)
 * + 127, the queue's tail standing at last_confirmed_frame - 1, input_queue.rs:83-101, :207 --,
 * a rollback to a frame that is not in the past
 * or older than the input queues hold, no connected player) or whose arrival row names a frame after its call (GGRS_E_INVALID) stops
 * there with that error (ggrs_p2p_read_sessions); the other sessions run on.  Kernel:
 * p2p_sched.hip. */
/* on = 1 switches the engine to arrival schedules; part of the configuration: before the first call */
int ggrs_p2p_set_arrival_schedule(ggrs_p2p_engine_t* eng, int32_t on);
/* arrive_upto [n_calls][num_sessions] i32: the newest remote frame delivered by each call (<= the
 * call's index; at or below what already arrived delivers nothing); events [n_calls][num_sessions]
 * u8 (NULL: none; bit k: Event::Disconnected of remote player k -- bits at or above num_players are
 * ignored, as the reference has no such player).  Calls in order from 0, at most input_capacity
 * calls ahead of the next call. */
int ggrs_p2p_add_arrivals(ggrs_p2p_engine_t* eng, int32_t first_call, int32_t n_calls, const int32_t* arrive_upto,
                          const uint8_t* events);
/* A peer's connect status as its input messages carry it (peer_connect_status): remote player
 * `reporter`'s endpoint reports remote player `player` disconnected with last frame `frame`
 * (-1 <= frame <= the call).  0 = no report. */
#define GGRS_PEER_REPORT(player, reporter, frame) (16 | (player) | (reporter) << 2 | ((frame) + 1) << 5)
/* reports [n_calls][num_sessions] i32 (GGRS_PEER_REPORT or 0) received by calls first_call ..
 * first_call + n_calls - 1, after their arrivals (ggrs_p2p_add_arrivals; calls not yet run).  A
 * report stands until its reporter disconnects; each call runs update_player_disconnects
 * (p2p_session.rs:748-783) over the standing ones: player k is disconnected at queue_min_confirmed
 * -- the oldest frame a running reporter gives, and k's own last frame while it is connected here
 * (endpoints that do not report k are taken to have seen every reported frame) -- when it is
 * connected here or its last frame is newer (the rollback then repeats every call, as the
 * reference's).  The repeat-last predictor only. */
int ggrs_p2p_add_peer_reports(ggrs_p2p_engine_t* eng, int32_t first_call, int32_t n_calls, const int32_t* reports);
/* per session: SyncLayer::current_frame, the calls that did not advance (prediction threshold),
 * and the session's error (0, GGRS_E_PRECONDITION or GGRS_E_INVALID); any pointer may be NULL */
int ggrs_p2p_read_sessions(ggrs_p2p_engine_t* eng, int32_t* frames, int32_t* skipped, int32_t* errors);
/* Desync detection under arrival schedules (p2p_session.rs:281-291, 904-975): for calls
 * first_call .. first_call + n_calls - 1 (run, and among the last input_capacity calls), per call and
 * session [n_calls][num_sessions]: the frame of the checksum report check_checksum_send_interval
 * sent (NULL_FRAME: none) and its checksum (the cell's, as read when sent), the
 * last_confirmed_frame compare_local_checksums_against_peers compared against in that call, and
 * the local players' last queued frame after the call (the reports travel with those inputs).
 * The pending-report bookkeeping and comparison are the caller's (ggrs_amd/desync.py
 * SchedDesyncDetector: UdpProtocol::on_checksum_report, protocol.rs:663-682) unless
 * ggrs_p2p_set_desync_compare hands them to the device (below).  A session whose
 * report cell is gone (the reference panics, :951-954) stops with GGRS_E_PRECONDITION.  Any output
 * pointer may be NULL. */
int ggrs_p2p_read_reports(ggrs_p2p_engine_t* eng, int32_t first_call, int32_t n_calls, int32_t* frames,
                          uint16_t* checksums, int32_t* last_confirmed, int32_t* local_last);

/* ---- Packet feed: the arrival schedules driven live.  A session's remote inputs enter as the
 * compressed Input messages its endpoint received (UdpProtocol::on_input,
 * src/network/protocol.rs:564-642), at the call that polled them, and the engine derives the
 * arrival rows itself.  The live loop per call: ggrs_p2p_add_inputs (the local players' bytes of row
 * c; the remote players' columns are ignored and hold arbitrary bytes until their packet arrives) ->
 * ggrs_p2p_receive_packets -> ggrs_p2p_advance_frames.  One packet carries one byte per remote player
 * per frame, ascending player order (InputBytes::to_player_inputs over the endpoint's handles); all
 * remote players of a session share one arrival stream, as in the arrival schedules.  ggrs_wire_unpack
 * (or the host) parses the Input message envelope (start_frame; ack_frame for its own send side; connect
 * status -> ggrs_p2p_add_peer_reports; disconnect_requested -> events).
 * Per session last_recv_frame starts at GGRS_NULL_FRAME; a packet (start, bytes) at call c:
 *  1. last_recv != NULL && last_recv + 1 < start is the reference's assert! (:588-590), and so is a
 *     first packet with start != 0: the session stops at call c with GGRS_E_PRECONDITION;
 *  2. the decode reference is the blank input while last_recv == NULL, else the remote bytes of frame
 *     start - 1, read from input row start - 1; the reference keeps frames >= last_recv -
 *     2 max_prediction (:636-639): an older one drops the packet (GGRS_PACKET_NO_REFERENCE), a kept
 *     one whose row slot holds another frame by now stops the session (GGRS_E_PRECONDITION) -- so
 *     input_capacity must cover 2 max_prediction + 1 frames behind last_recv plus the session's lag;
 *  3. compression::decode with ggrs_codec_decode's acceptance and codes; a rejected packet is dropped
 *     whole (more than max_packet_inputs inputs: GGRS_CODEC_E_CAP);
 *  4. frames <= last_recv are skipped, the later ones stored into the remote columns of their rows,
 *     last_recv = the packet's last frame; a frame whose row slot holds another frame stops the
 *     session (GGRS_E_PRECONDITION), a last frame beyond the call index stops it with GGRS_E_INVALID
 *     (the arrival rows' rule: remote and local inputs share a row, so a live host runs its sessions
 *     no further ahead than its peers);
 *  5. the call's arrival row is last_recv.
 * A stopped session receives nothing more.  Kernel: p2p_ingest.hip. */
#define GGRS_PACKET_NO_REFERENCE (-16) /* dropped: the decode reference (frame start - 1) is no longer kept */
#define GGRS_PACKET_STOPPED (-17)      /* this packet stopped the session (ggrs_p2p_read_sessions has the error) */
/* Part of the configuration (after ggrs_p2p_set_arrival_schedule(eng, 1), before the first call and
 * the first arrivals): max_packet_inputs in 1..128 (PENDING_OUTPUT_SIZE, protocol.rs:22),
 * packet_stride a multiple of 4, >= ggrs_codec_max_packet_bytes(remote players, max_packet_inputs)
 * and <= 1012.  From then on ggrs_p2p_add_arrivals returns GGRS_E_STATE. */
int ggrs_p2p_set_packet_feed(ggrs_p2p_engine_t* eng, int32_t max_packet_inputs, int32_t packet_stride);
/* The packets polled by calls first_call .. first_call + n_calls - 1 (in call order, as
 * ggrs_p2p_add_arrivals; their input rows already added): start_frame [n_calls][num_sessions] i32
 * (negative: no packet), packet_len [n][S] i32, packets [n][S][packet_stride] u8, events [n][S] u8 as
 * ggrs_p2p_add_arrivals' (NULL: none; bits at or above num_players ignored); at most one packet per session and call, the newest of the
 * poll (a sender repeats everything unacknowledged).  on_device: the four pointers are device
 * memory (packets dword aligned), read by a launch on the engine's stream; else host memory.
 * GGRS_E_STATE without ggrs_p2p_set_packet_feed. */
int ggrs_p2p_receive_packets(ggrs_p2p_engine_t* eng, int32_t first_call, int32_t n_calls,
                             const int32_t* start_frame, const int32_t* packet_len, const uint8_t* packets,
                             const uint8_t* events, int32_t on_device);
/* For received calls among the last input_capacity, [n_calls][num_sessions] each (either may be
 * NULL): status 1 = decoded and delivered at least one new frame, 0 = no packet or nothing new, a
 * GGRS_CODEC_E_* / GGRS_CODEC_UNSUPPORTED code = dropped as undecodable, GGRS_PACKET_NO_REFERENCE,
 * GGRS_PACKET_STOPPED; ack_frame = last_recv_frame after the call (what send_input_ack carries). */
int ggrs_p2p_read_packet_results(ggrs_p2p_engine_t* eng, int32_t first_call, int32_t n_calls, int32_t* status,
                                 int32_t* ack_frame);

/* ---- Packet emit: the send side of the same endpoint.  Every session's outgoing Input message body
 * is built on the device from the engine's own input rows: UdpProtocol::send_input
 * (src/network/protocol.rs:421-448), send_pending_output (:450-487), pop_pending_output (:378-391, from
 * on_input :566 and on_input_ack :644-646) and poll's retry (:333-337), called from
 * P2PSession::advance_frame (p2p_session.rs:363-387) and poll_remote_clients (:430-478).  One endpoint
 * per session holds all of its remote players; arrival-schedule mode is required, the packet feed is
 * not; rollback and lockstep mode.  One pending input is one byte per local player of one frame,
 * ascending player order (InputBytes::from_inputs, protocol.rs:52-80).  Per session last_acked starts
 * as (GGRS_NULL_FRAME, zero bytes), pending empty, the stream open.  Call c, after it ran:
 *  1. ack_in[c], the newest ack_frame the call's poll received (an Input message's or a bare
 *     InputAck's; GGRS_NULL_FRAME: none), pops every pending input with frame <= it; last_acked
 *     becomes the last one popped (a stale ack changes nothing; one beyond the newest pending frame
 *     pops everything and last_acked is that newest pending input);
 *  2. an events bit of a remote player at call c (Event::Disconnected -> disconnect_player_at_frame ->
 *     endpoint.disconnect(), p2p_session.rs:618-655) closes the stream: GGRS_EMIT_CLOSED, nothing is
 *     emitted from this call on.  Peer reports do not close it.  Divergence: the closing call itself
 *     emits nothing, where the reference's poll could still send a timer retry before the event;
 *  3. if call c's add_local_input was accepted (the local players' last queued frame rose: not at the
 *     prediction threshold's repeat, not a lockstep call that waits), frame current_frame + input_delay
 *     is pushed with the local columns of input row c; more than max_pending_inputs pending closes the
 *     stream with GGRS_EMIT_DISCONNECTED -- the Event::Disconnected of :443-445, applied at once
 *     (divergence: the reference's session handles it in its next poll); the overflowing call emits
 *     nothing;
 *  4. a packet goes out when a frame was pushed, or when resend[c] is set (the host's 200 ms retry
 *     timer) and something is pending; at most one per call: start_frame = the first pending frame,
 *     bytes = compression::encode(last_acked's bytes, the pending inputs), as ggrs_codec_encode;
 *  5. ack_frame[c] = the endpoint's last_recv_frame after call c (the packet feed's, or the newest frame
 *     of the arrival rows), written for every call: what the Input message or a bare InputAck carries;
 *  6. a session that stopped (an error in ggrs_p2p_read_sessions) emits nothing from its stopping call on.
 * ggrs_wire_pack (or the host) fills the envelope: peer_connect_status and disconnect_requested.  With emit
 * configured the scheduled kernels store one more word per session and call.  Kernel: p2p_emit.hip. */
#define GGRS_EMIT_CLOSED (-18)        /* the stream closed on an Event::Disconnected of a remote player */
#define GGRS_EMIT_DISCONNECTED (-19)  /* more than max_pending_inputs unacknowledged inputs */
/* Part of the configuration (after ggrs_p2p_set_arrival_schedule(eng, 1), before the first call; a
 * local and a remote player): max_pending_inputs in 1..128 (PENDING_OUTPUT_SIZE, protocol.rs:22),
 * out_stride a multiple of 4, >= ggrs_codec_max_packet_bytes(local players, max_pending_inputs) and
 * <= 1012.  GGRS_E_STATE after the first call. */
int ggrs_p2p_set_packet_emit(ggrs_p2p_engine_t* eng, int32_t max_pending_inputs, int32_t out_stride);
/* Calls first_call .. first_call + n_calls - 1: already run, in order, each exactly once, still among
 * the last input_capacity calls (GGRS_E_INVALID otherwise).  ack_in [n][S] i32 and resend [n][S] u8 may
 * be NULL (none).  Outputs: start_frame [n][S] (-1: no packet), packet_len [n][S] (0: none), ack_frame
 * [n][S], packets [n][S][out_stride]; bytes past packet_len are unspecified.  on_device: every
 * pointer is device memory (packets dword aligned), written by a launch on the engine's stream; the
 * caller orders its consumer after that launch.  The result does not depend on how the calls are
 * split over ggrs_p2p_emit_packets.  GGRS_E_STATE without ggrs_p2p_set_packet_emit. */
int ggrs_p2p_emit_packets(ggrs_p2p_engine_t* eng, int32_t first_call, int32_t n_calls, const int32_t* ack_in,
                          const uint8_t* resend, int32_t* start_frame, int32_t* packet_len, int32_t* ack_frame,
                          uint8_t* packets, int32_t on_device);
/* Per session, [num_sessions] each (any may be NULL): last_acked's frame, the pending count, the status
 * (0 open, GGRS_EMIT_CLOSED, GGRS_EMIT_DISCONNECTED) and the call at which the stream closed (-1). */
int ggrs_p2p_read_emit_state(ggrs_p2p_engine_t* eng, int32_t* last_acked, int32_t* pending, int32_t* status,
                             int32_t* closed_call);

/* ---- Spectator emit: every session's confirmed inputs as the Input message bodies its host sends to
 * its spectators, built on the device: P2PSession::send_confirmed_inputs_to_spectators
 * (p2p_session.rs:716-745) with SyncLayer::confirmed_inputs (sync_layer.rs:296-310), and per spectator
 * endpoint UdpProtocol::send_input (protocol.rs:421-448), send_pending_output (:450-487),
 * pop_pending_output (:378-391) and poll's retry (:333-337).  K = num_spectators endpoints per session.
 * Arrival-schedule mode is required; sparse saving, lockstep mode, the packet feed and packet emit
 * combine with it; peers' disconnect reports do not (GGRS_E_STATE from whichever comes second).  One
 * pending input is num_players bytes of one frame in ascending player order, the row
 * ggrs_spectator_add_inputs takes.  Per session next_spectator_frame starts at 0; per endpoint
 * last_acked = (GGRS_NULL_FRAME, zero bytes), pending empty, the stream open.  Call c, after it ran:
 *  1. ack_in[c][k], the newest InputAck from spectator k (GGRS_NULL_FRAME: none), pops that endpoint's
 *     pending inputs with frame <= it; last_acked becomes the last one popped (stale acks and acks
 *     beyond the newest pending frame as in ggrs_p2p_emit_packets);
 *  2. confirmed = the call's confirmed_frame() (:542-553): the minimum over connected players of the
 *     local players' last queued frame before this call's add_local_input and of the remote players'
 *     last received frame, under the connect status after the call's poll.  Every frame f in
 *     [next_spectator_frame, confirmed] is pushed to every open endpoint -- a burst may confirm many
 *     in one call: player k's byte is zero when disconnected[k] && last_frame[k] < f (blank_input),
 *     else its confirmed input of frame f (a remote player's from input row f, a local player's from
 *     the row of the call that queued frame f); next_spectator_frame = confirmed + 1;
 *  3. more than max_pending_inputs pending on an endpoint closes it with GGRS_EMIT_DISCONNECTED (the
 *     Event::Disconnected of :443-445), applied at once; the call emits nothing for it (divergence,
 *     as packet emit's); the session's other endpoints go on;
 *  4. an endpoint emits when the call pushed at least one frame, or resend[c][k] is set and something
 *     is pending: start_frame = its first pending frame, bytes = compression::encode(last_acked's
 *     bytes, the pending inputs), as ggrs_codec_encode.  Divergence: the reference queues one message
 *     per pushed frame, each a superset of the one before; this is the last of them, all that a
 *     receiver taking the newest packet of its poll needs;
 *  5. notes[c] is the messages' peer_connect_status as ggrs_spectator_receive_packets takes it: 0 while
 *     no player is disconnected; one disconnected player's GGRS_SPECTATOR_NOTE(player, last_frame) on
 *     every call from its disconnect on; with m > 1 disconnected players the (c mod m)-th of them in
 *     ascending player order (divergence: every reference message carries the whole status, here a
 *     spectator learns of a player at most num_players - 1 delivered packets late; the merge is
 *     sticky, so repetition is harmless);
 *  6. a session that stopped (an error in ggrs_p2p_read_sessions) pushes and emits nothing from its
 *     stopping call on (its notes are 0);
 *  7. a frame to push that reads its input row (a remote player's byte that is not blank) whose row is
 *     no longer among the input_capacity rows held closes the
 *     session's open endpoints with GGRS_EMIT_ROW_LOST, and the session pushes nothing from that call
 *     on: the emit was called too late for this input_capacity.  Emitting call c needs the rows from
 *     next_spectator_frame on, so emit before more than input_capacity - (the longest arrival stall in
 *     calls) - 1 further rows are added.
 * The Input envelope's ack_frame and disconnect_requested are ggrs_wire_pack's or the host's (a spectator
 * sends no inputs).  The scheduled kernels store what they store for packet emit, one word per session and
 * call; confirmed_frame and the connect status are restated by the emit from that word, the arrival
 * rows and the events.  Kernel: p2p_spec_emit.hip. */
#define GGRS_EMIT_ROW_LOST (-20)  /* an input row to push was overwritten before the emit read it */
/* Part of the configuration (after ggrs_p2p_set_arrival_schedule(eng, 1), before the first call and
 * before any peer report; a local player): num_spectators in 1..4, max_pending_inputs in 1..128,
 * out_stride a multiple of 4, >= ggrs_codec_max_packet_bytes(num_players, max_pending_inputs) and
 * <= 1012 (GGRS_E_INVALID otherwise).  GGRS_E_STATE after the first call, on a fixed-latency engine
 * and with peer reports. */
int ggrs_p2p_set_spectator_emit(ggrs_p2p_engine_t* eng, int32_t num_spectators, int32_t max_pending_inputs,
                                int32_t out_stride);
/* Calls first_call .. first_call + n_calls - 1: already run, in order, each exactly once, still among
 * the last input_capacity calls (GGRS_E_INVALID otherwise).  With K = num_spectators and S =
 * num_sessions: ack_in [n][K][S] i32 and resend [n][K][S] u8 may be NULL (none).  Outputs: start_frame
 * [n][K][S] (-1: no packet), packet_len [n][K][S] (0: none), notes [n][S], packets
 * [n][K][S][out_stride]; bytes past packet_len are unspecified.  For n = 1 the slices of one k are the
 * arrays ggrs_spectator_receive_packets reads.  on_device as ggrs_p2p_emit_packets.  The result does not
 * depend on how the calls are split over invocations.  GGRS_E_STATE without
 * ggrs_p2p_set_spectator_emit. */
int ggrs_p2p_emit_spectator_packets(ggrs_p2p_engine_t* eng, int32_t first_call, int32_t n_calls,
                                    const int32_t* ack_in, const uint8_t* resend, int32_t* start_frame,
                                    int32_t* packet_len, int32_t* notes, uint8_t* packets, int32_t on_device);
/* next_spectator_frame [S]; per endpoint [K][S] each: last_acked's frame, the pending count (frozen
 * at max_pending_inputs + 1 by an overflow), the status (0 open, GGRS_EMIT_DISCONNECTED,
 * GGRS_EMIT_ROW_LOST) and the call at which the endpoint closed (-1).  Any pointer may be NULL. */
int ggrs_p2p_read_spectator_emit_state(ggrs_p2p_engine_t* eng, int32_t* next_spectator_frame, int32_t* last_acked,
                                       int32_t* pending, int32_t* status, int32_t* closed_call);

/* ---- Time sync: every session's P2PSession::frames_ahead() and GgrsEvent::WaitRecommendation, per
 * call, on the device: check_wait_recommendation (p2p_session.rs:357, :804-817) over max_frame_advantage
 * (:786-802), the endpoint's TimeSync window (time_sync.rs:25-39), update_local_frame_advantage
 * (protocol.rs:260-269, from poll_remote_clients, p2p_session.rs:442-447), on_quality_report
 * (protocol.rs:649-653), on_quality_reply and the window push inside send_input (:433-437).  One
 * endpoint per session holds all of its remote players, as in packet emit.  Arrival-schedule mode is
 * required; lockstep mode, the packet feed and the two emits combine with it; peers' disconnect reports
 * do not (GGRS_E_STATE from whichever comes second: the connect status is restated from the events bits
 * alone).  Per session round_trip_time (ms), remote_frame_advantage, local_frame_advantage and
 * next_recommended_sleep start at 0, the two windows of 30 entries at zeros, the endpoint open.  Call c,
 * after it ran:
 *  1. a session that stopped (an error in ggrs_p2p_read_sessions) takes no step from its stopping call
 *     on: frames_ahead 0, skip_frames 0, local_advantage its last value;
 *  2. while the endpoint is open, rtt_ms[c] >= 0 sets round_trip_time (a negative value keeps it; values
 *     above 1 << 20 are clamped there -- divergence: the reference overflows only beyond i32, the clamp
 *     keeps ping * fps inside i32), and remote_advantage[c] != GGRS_TIME_SYNC_KEEP sets
 *     remote_frame_advantage, clamped to the i16 range as send_quality_report clamps what it sends
 *     (protocol.rs:504-508) -- so one engine's local_advantage row is its peer's remote_advantage row;
 *  3. while the endpoint is open and last_recv_frame != GGRS_NULL_FRAME: local_frame_advantage =
 *     last_recv_frame + ((round_trip_time / 2) * fps) / 1000 - current_frame, with current_frame that of
 *     the call's start and last_recv_frame the endpoint's after the call's poll (ack_frame of
 *     ggrs_p2p_emit_packets);
 *  4. an Event::Disconnected bit of a remote player at call c closes the endpoint from here on
 *     (disconnect_player_at_frame, :618-655): nothing is taken in or pushed any more;
 *  5. frames_ahead[c] = average_frame_advantage() while the endpoint is open, else 0: from the windows
 *     before this call's push, in f32 as time_sync.rs:30-39 (local_sum / 30.0, remote_sum / 30.0,
 *     (remote_avg - local_avg) / 2.0 truncated).  If current_frame > next_recommended_sleep and
 *     frames_ahead >= 3 (MIN_RECOMMENDATION): next_recommended_sleep = current_frame + 60
 *     (RECOMMENDATION_INTERVAL) and skip_frames[c] = frames_ahead; else skip_frames[c] = 0;
 *  6. while the endpoint is open and the call's add_local_input was accepted:
 *     local[(current_frame + input_delay) % 30] = local_frame_advantage, remote[...] =
 *     remote_frame_advantage;
 *  7. local_advantage[c] = local_frame_advantage after the call: NetworkStats::local_frames_behind, and
 *     what a QualityReport sent at this call carries.
 * Not built: the recommendation is reported, not enacted (every session of an engine takes every call);
 * the QualityReport / QualityReply messages are ggrs_wire_unpack's and ggrs_wire_pack's, their 200 ms
 * timer is ggrs_p2p_poll_endpoints' send_report; NetworkStats' send_queue_len and kbps_sent stay with the
 * host; fixed-latency engines and peer reports.
 * The scheduled kernels store what they store for packet emit, one word per session and call.
 * Kernel: p2p_time_sync.hip. */
#define GGRS_TIME_SYNC_KEEP INT32_MIN /* remote_advantage: no QualityReport arrived at this call */
/* Part of the configuration (after ggrs_p2p_set_arrival_schedule(eng, 1), before the first call and
 * before any peer report; a local and a remote player): fps in 1..1000 (the reference's default: 60;
 * GGRS_E_INVALID otherwise).  GGRS_E_STATE after the first call, on a fixed-latency engine and with peer
 * reports. */
int ggrs_p2p_set_time_sync(ggrs_p2p_engine_t* eng, int32_t fps);
/* Calls first_call .. first_call + n_calls - 1: already run, in order, each exactly once, still among
 * the last input_capacity calls (GGRS_E_INVALID otherwise).  rtt_ms [n][S] and remote_advantage [n][S]
 * may be NULL (nothing arrived).  Outputs [n][S] each: local_advantage, frames_ahead, skip_frames.
 * on_device as ggrs_p2p_emit_packets.  The result does not depend on how the calls are split over
 * invocations.  GGRS_E_STATE without ggrs_p2p_set_time_sync. */
int ggrs_p2p_time_sync(ggrs_p2p_engine_t* eng, int32_t first_call, int32_t n_calls, const int32_t* rtt_ms,
                       const int32_t* remote_advantage, int32_t* local_advantage, int32_t* frames_ahead,
                       int32_t* skip_frames, int32_t on_device);
/* Per session, [num_sessions] each: local_frame_advantage, remote_frame_advantage, round_trip_time,
 * next_recommended_sleep and the call at which the endpoint closed (-1: open); windows [2][30][S], the
 * local window then the remote one.  Any pointer may be NULL. */
int ggrs_p2p_read_time_sync_state(ggrs_p2p_engine_t* eng, int32_t* local_advantage, int32_t* remote_advantage,
                                  int32_t* rtt_ms, int32_t* next_recommended_sleep, int32_t* closed_call,
                                  int32_t* windows);

/* ---- Checksum comparison: the receive side of desync detection under arrival schedules, every
 * session's GgrsEvent::DesyncDetected on the device: UdpProtocol::on_checksum_report
 * (protocol.rs:663-682) and compare_local_checksums_against_peers (p2p_session.rs:904-937) with the
 * history push of check_checksum_send_interval (:965-970), over the report rows the scheduled kernels
 * store (ggrs_p2p_read_reports) and the peer's.  One endpoint per session holds all of its remote
 * players, as in packet emit.  Arrival-schedule mode and ggrs_p2p_set_desync_detection(interval > 0) are
 * required; lockstep mode (which sends no report), the packet feed, the emits and time sync combine with
 * it.  Per session local_checksum_history and pending_checksums hold at most 32 (frame, u16 checksum)
 * entries (MAX_CHECKSUM_HISTORY_SIZE, protocol.rs:27), both empty at first.  Call c, after it ran:
 *  1. delivery: the peer's rows g = (rows delivered so far), .. while g < c and local_last of the peer's
 *     row g (the inputs its report travelled with) <= last_recv_frame of call c -- the feed's ack_frame
 *     with the packet feed, else the running maximum of the arrival rows.  A row with frame >= 0 is
 *     on_checksum_report: with 32 reports pending those with frame < frame - 31 interval are dropped
 *     first, then the report is inserted.  Divergence: a report whose frame is not a positive multiple of
 *     the interval, or not above the newest frame received from the peer so far, is refused and counted
 *     (the reference accepts any frame; a peer of the same configuration sends no such report), so the
 *     table never exceeds 32 entries;
 *  2. the call's own report (frame >= 0) enters the history; a 33rd entry prunes it to frames >=
 *     frame - 31 interval;
 *  3. every pending report, in ascending frame order (the reference iterates a HashMap), with frame <
 *     the call's last_confirmed and its frame in the history is compared and removed; a difference is a
 *     DesyncDetected: (call, session, frame, local checksum, remote checksum);
 *  4. a session that stopped takes its rows as ggrs_p2p_read_reports returns them (no report).  A
 *     session whose next row to deliver is more than input_capacity rows behind the rows added when
 *     ggrs_p2p_compare_reports is called has lost that row to the ring: its status becomes
 *     GGRS_DESYNC_ROW_LOST and it takes no step and raises nothing from that invocation's first call on;
 *     the other sessions go on.
 * Events go to a list of max_events records; the count stays exact when the list is full (which records
 * a full list keeps is unspecified), and so does the per-session summary.  The ChecksumReport message
 * envelope is ggrs_wire_unpack's and ggrs_wire_pack's.  Not built: several endpoints per session, fixed-latency engines (ggrs_p2p_compare_checksums).
 * The scheduled kernels store nothing new.  Kernel: p2p_desync.hip. */
#define GGRS_DESYNC_ROW_LOST (-21)  /* a peer's report row was overwritten before the session read it */
/* Part of the configuration (after ggrs_p2p_set_arrival_schedule(eng, 1) and
 * ggrs_p2p_set_desync_detection(eng, interval > 0), before the first call): max_events in 1..2^26
 * (GGRS_E_INVALID otherwise).  GGRS_E_STATE after the first call, on a fixed-latency engine and without
 * desync detection. */
int ggrs_p2p_set_desync_compare(ggrs_p2p_engine_t* eng, int32_t max_events);
/* The peer's ggrs_p2p_read_reports rows (frames, checksums, local_last; [n][S] each) of its calls
 * first_call .. first_call + n_calls - 1: in call order from 0, n_calls <= input_capacity (GGRS_E_INVALID
 * otherwise).  on_device != 0: device pointers, copied on the engine's stream.  The engine keeps the last
 * input_capacity rows. */
int ggrs_p2p_add_remote_reports(ggrs_p2p_engine_t* eng, int32_t first_call, int32_t n_calls, const int32_t* frames,
                                const uint16_t* checksums, const int32_t* local_last, int32_t on_device);
/* The same rows straight from the peer engine's report rows, device to device: calls the peer has run
 * that are among its last input_capacity (GGRS_E_INVALID otherwise); the same sessions on the same
 * device.  The copy waits for the peer's launches and the peer's next launch for the copy. */
int ggrs_p2p_add_remote_reports_from(ggrs_p2p_engine_t* eng, ggrs_p2p_engine_t* peer_eng, int32_t first_call,
                                     int32_t n_calls);
/* Steps 1-4 for calls first_call .. first_call + n_calls - 1: already run, in order, each exactly once,
 * still among the last input_capacity calls (GGRS_E_INVALID otherwise).  GGRS_E_STATE, naming the
 * missing call, unless the peer's rows through call first_call + n_calls - 2 were added: no report is
 * ever delivered later than the reference delivers it.  n_events_total (may be NULL: then the call does
 * not wait for the launch): the events raised so far, by every invocation.  The events and the state do
 * not depend on how the calls are split over invocations (GGRS_DESYNC_ROW_LOST does: it is found where
 * an invocation starts). */
int ggrs_p2p_compare_reports(ggrs_p2p_engine_t* eng, int32_t first_call, int32_t n_calls, int32_t* n_events_total);
/* Records first .. first + max - 1 of the event list, in the order they were appended (unspecified
 * within an invocation): n_read of them (at most max_events exist).  Any array may be NULL. */
int ggrs_p2p_read_desync_events(ggrs_p2p_engine_t* eng, int32_t first, int32_t max, int32_t* call, int32_t* session,
                                int32_t* frame, uint16_t* local, uint16_t* remote, int32_t* n_read);
/* Per session, [num_sessions] each: status (0, GGRS_DESYNC_ROW_LOST), the events raised, the first
 * event's call (-1: none), frame (-1), local and remote checksum, the reports refused; history and
 * pending [2][32][S] each: the entries' frames in ascending order (-1 past the last), then their
 * checksums (0).  Any pointer may be NULL. */
int ggrs_p2p_read_desync_state(ggrs_p2p_engine_t* eng, int32_t* status, int32_t* n_events, int32_t* first_call,
                               int32_t* first_frame, int32_t* first_local, int32_t* first_remote, int32_t* refused,
                               int32_t* history, int32_t* pending);

/* ---- Endpoint poll: every session's UdpProtocol::poll (protocol.rs:329-376) with the clock bookkeeping
 * of handle_message (:534-551), per call, on the device: the 200 ms retry and quality-report timers
 * (RUNNING_RETRY_INTERVAL, QUALITY_REPORT_INTERVAL, :17-19), GgrsEvent::NetworkInterrupted and
 * NetworkResumed, the disconnect timeout's Event::Disconnected and the endpoint's way from Running over
 * Disconnected to Shutdown (disconnect, :311-319; UDP_SHUTDOWN_TIMER 5000 ms, :21).  One endpoint per
 * session holds all of its remote players, as in packet emit.  Arrival-schedule mode is required;
 * lockstep mode, sparse saving, the packet feed, both emits, time sync, the comparison and peers'
 * disconnect reports combine with it.  Per session last_recv_time, running_last_input_recv,
 * running_last_quality_report and shutdown_timeout start at start_ms (every Instant of UdpProtocol::new,
 * :219-220, :227, :252), the state Running, disconnect_notify_sent and disconnect_event_sent false.
 * All times are u64 milliseconds, nothing is truncated to 32 bits; `<` is strict, as in the reference.
 * Call c's poll at clock now = now_ms[c], after call c's arrivals were added or its packets received
 * and before the call runs:
 *  0. Shutdown: every output 0, nothing changes (:538-541, :373);
 *  1. k = kinds[c] != 0 (a message was accepted): last_recv_time = now; with disconnect_notify_sent set
 *     and the state Running the flag is cleared and GGRS_NET_RESUMED raised (:544-551);
 *  2. decoded = k has the Input bit and, with the packet feed, the feed's status of call c
 *     (ggrs_p2p_read_packet_results) is >= 0: running_last_input_recv = now, send_ack[c] = 1 (:608, :634);
 *  3. ext = the call's events byte holds a remote player's bit (a received disconnect_requested, or the
 *     host's own);
 *  4. while Running, in poll()'s order: (a) running_last_input_recv + 200 < now: resend[c] = 1,
 *     running_last_input_recv = now, whether or not anything is pending (emit decides that); (b)
 *     running_last_quality_report + 200 < now: send_report[c] = 1, running_last_quality_report = now;
 *     (c) !disconnect_notify_sent and last_recv_time + disconnect_notify_start < now:
 *     GGRS_NET_INTERRUPTED, the flag set; (d) ext sets disconnect_event_sent; else with the flag clear
 *     and last_recv_time + disconnect_timeout < now: GGRS_NET_DISCONNECTED, the flag set, the remote
 *     players' bits OR-ed into the engine's events row of call c on the device, ext = 1; (e) ext: the
 *     state becomes Disconnected, shutdown_timeout = now + 5000, closed_call = c;
 *  5. Disconnected at entry: steps 1-3 apply (acks keep flowing, nothing resumes), the timers do not;
 *     shutdown_timeout < now: the state becomes Shutdown, GGRS_NET_SHUTDOWN raised.
 * The scheduled kernels, both emits and time sync read the events row, so a timed-out player is
 * disconnected by call c itself (disconnect_player_at_frame, p2p_session.rs:618-655: the rollback that
 * replays the player as InputStatus::Disconnected) and the other units close their endpoint at c; a
 * stopped session gets no special case.  There is no keep_alive output because send_keep_alive
 * (:344-347) cannot fire: last_send_time is set by every queue_message (:523), send_quality_report sets
 * running_last_quality_report and then queues (:502, :512), and the constructor initialises the two in
 * that order, so last_send_time >= running_last_quality_report at every check; both intervals are
 * 200 ms, so either the report fired in this poll and last_send_time is later than poll's now, or
 * last_send_time + 200 >= running_last_quality_report + 200 >= now.  ggrs_wire_pack's keep_alive input
 * stays a caller's option.
 * Stated divergences: one clock per poll stands for the reference's several Instant::now() reads; a
 * remote bit given to an endpoint that is already Disconnected changes nothing (the reference cannot
 * raise a second Event::Disconnected); after Shutdown send_all_messages drops the queue (:401-407) --
 * the host drops what the other units still produce, by `state`; a player disconnected through a peer's
 * report (ggrs_p2p_add_peer_reports) reaches endpoint.disconnect() in the reference
 * (disconnect_player_at_frame, p2p_session.rs:618-652), but the unit reads the events byte alone, so its
 * endpoint stays Running, its timers keep firing and it can still raise GGRS_NET_INTERRUPTED or
 * GGRS_NET_DISCONNECTED later -- the two modes run side by side, untested together; a host that wants
 * the reference's endpoint puts the remote players' bits into that call's events byte as well.
 * A limit of the input rows, not of this unit: a link that stays silent keeps the row of the last frame
 * it delivered in use (the repeat-last prediction's base), and once input_capacity further rows have
 * been added over it the scheduled launch stops the session with GGRS_E_PRECONDITION, where the
 * reference plays on.  The timeout ends that wait only if it comes first: keep input_capacity above the
 * calls that disconnect_timeout_ms spans, plus the calls queued ahead.  A session whose remote players
 * were all disconnected while its link was silent still holds that row: it stops input_capacity calls
 * after the silence began, so a server retires a timed-out match before then.  The spectator endpoints'
 * poll is "Spectator endpoint poll" below, the spectator engine's own "Spectator engine: endpoint poll".
 * Not built: NetworkStats::kbps_sent (it sums size_of_val(&Message), a Rust
 * layout).  The unit reports per call; the sessions' GgrsEvent queues with MAX_EVENT_QUEUE_SIZE are
 * "Event queue" below, which takes the net_events row.
 * Kernel: p2p_poll.hip (the step: poll_device.h). */
#define GGRS_NET_INTERRUPTED 1  /* Event::NetworkInterrupted at this call (its payload: disconnect_timeout - notify_start) */
#define GGRS_NET_RESUMED 2      /* Event::NetworkResumed */
#define GGRS_NET_DISCONNECTED 4 /* Event::Disconnected raised by the disconnect timeout at this call */
#define GGRS_NET_SHUTDOWN 8     /* the endpoint went Disconnected -> Shutdown at this call */
#define GGRS_ENDPOINT_RUNNING 0
#define GGRS_ENDPOINT_DISCONNECTED 1
#define GGRS_ENDPOINT_SHUTDOWN 2
/* Part of the configuration (after ggrs_p2p_set_arrival_schedule(eng, 1), before the first call; a local
 * and a remote player): the reference's defaults are 2000 and 500 ms (builder.rs:17-18).
 * disconnect_notify_start_ms > disconnect_timeout_ms is GGRS_E_INVALID (the reference's Duration
 * subtraction at :353 panics).  GGRS_E_STATE after the first call and on a fixed-latency engine.  From
 * then on ggrs_p2p_advance_frames returns GGRS_E_STATE, naming the call, for a call that was not polled:
 * a timeout is never delivered later than the reference delivers it. */
int ggrs_p2p_set_endpoint_poll(ggrs_p2p_engine_t* eng, uint64_t disconnect_timeout_ms,
                               uint64_t disconnect_notify_start_ms, uint64_t start_ms);
/* The polls of calls first_call .. first_call + n_calls - 1: in order, each exactly once, not yet run
 * (first_call >= ggrs_p2p_calls), their arrivals added or packets received (GGRS_E_INVALID otherwise,
 * nothing launched).  now_ms [n] u64 never decreases: a host array that does (or starts below the last
 * host clock) is GGRS_E_INVALID; on the device a value below the engine's last clock, which is kept in
 * device memory, is taken as that clock.  kinds [n][S] u8 as ggrs_wire_unpack writes it (NULL: nothing
 * arrived).  Outputs [n][S] u8 each, any may be NULL: resend (ggrs_p2p_emit_packets' input), send_ack and
 * send_report (ggrs_wire_pack's), net_events (GGRS_NET_* bits).  on_device as ggrs_p2p_emit_packets.
 * The result does not depend on how the calls are split over invocations.  GGRS_E_STATE without
 * ggrs_p2p_set_endpoint_poll. */
int ggrs_p2p_poll_endpoints(ggrs_p2p_engine_t* eng, int32_t first_call, int32_t n_calls, const uint64_t* now_ms,
                            const uint8_t* kinds, uint8_t* resend, uint8_t* send_ack, uint8_t* send_report,
                            uint8_t* net_events, int32_t on_device);
/* Per session, [num_sessions] each: the state (GGRS_ENDPOINT_*), the four times, flags (bit 0
 * disconnect_notify_sent, bit 1 disconnect_event_sent) and the call at which the endpoint left Running
 * (-1).  Any pointer may be NULL. */
int ggrs_p2p_read_endpoint_state(ggrs_p2p_engine_t* eng, int32_t* state, uint64_t* last_recv_ms,
                                 uint64_t* last_input_recv_ms, uint64_t* last_report_ms, uint64_t* shutdown_ms,
                                 int32_t* flags, int32_t* closed_call);

/* ---- Spectator endpoint poll: the same for the num_spectators endpoints a session has towards its
 * spectators (ggrs_p2p_set_spectator_emit is their send side): P2PSession::poll_remote_clients'
 * spectator loop (p2p_session.rs:458-464) with handle_event (:866-878), disconnect_player (:506-509)
 * and disconnect_player_at_frame's spectator branch (:645-652), on the device.  Every array is
 * [n][K][S], K = num_spectators; times, strictness and the start values are "Endpoint poll"'s.
 * Endpoint k of session s at call c, at clock now = max(now_ms[c], the engine's last clock):
 *  0. Shutdown: every output 0, nothing changes;
 *  1. kinds[c][k] != 0: last_recv_time = now; GGRS_NET_RESUMED while Running with
 *     disconnect_notify_sent set, the flag cleared.  A spectator sends no Input: an Input bit counts as a
 *     message and nothing else, and there is no send_ack output.  Stated divergence: the reference would
 *     decode it and then hit the assert! of p2p_session.rs:882;
 *  2. ext has two sources: close_in[c][k] != 0, the host's own disconnect_player(spectator), which
 *     raises no event; and spectator emit having closed this endpoint with GGRS_EMIT_DISCONNECTED at a
 *     call before c -- the Event::Disconnected send_input queues (protocol.rs:443-445), which the
 *     reference handles at the next poll, so GGRS_NET_DISCONNECTED is raised here.  Neither sets
 *     disconnect_event_sent (the reference's paths do not);
 *  3. while Running, in poll()'s order: (a) running_last_input_recv + 200 < now: resend[c][k] = 1 and
 *     the time reset -- nothing else ever resets it for a spectator, so the retry recurs every time more
 *     than 200 ms have passed; (b) send_report as in "Endpoint poll"; (c) GGRS_NET_INTERRUPTED; (d) with
 *     disconnect_event_sent clear and last_recv_time + disconnect_timeout < now: GGRS_NET_DISCONNECTED,
 *     the flag set, ext = 1; (e) ext: the state becomes Disconnected, shutdown_timeout = now + 5000,
 *     closed_call = c;
 *  4. Disconnected at entry: shutdown_timeout < now gives Shutdown and GGRS_NET_SHUTDOWN.
 * A spectator's timeout does not enter the game: no events row is written, the session and its other
 * endpoints are untouched.  What spectator emit reads: an endpoint whose closed_call is >= 0 and <= c
 * pushes and emits nothing from call c on, a resend included; its emit status becomes GGRS_EMIT_CLOSED
 * and its emit closing call the poll's (send_input's early return and the is_running() check,
 * protocol.rs:426, p2p_session.rs:736).  With the unit on, ggrs_p2p_emit_spectator_packets returns
 * GGRS_E_STATE, naming the call, for a call whose spectator endpoints were not polled; the order within
 * a call is otherwise free, and no ordering against ggrs_p2p_advance_frames is needed.
 * Stated limit: the overflow of step 2 is seen as of the launch.  It lands at the reference's call when
 * each call's emit precedes the next call's poll (the live loop); polled further ahead, it lands at the
 * next launch's first call.  At the reference's defaults the 2000 ms timeout precedes the 128-input
 * overflow at 60 fps, so this is a backstop.  Everything else is independent of how the calls are split.
 * No keep-alive row: see "Endpoint poll"; the argument does not depend on who the peer is.  Out of scope:
 * NetworkStats (kbps_sent, send_queue_len), fixed-latency engines, peers' disconnect reports (the
 * GgrsEvent queue with MAX_EVENT_QUEUE_SIZE is "Event queue" below, which takes the net_events rows).
 * Measured (profiles/spectator_poll_rate.json): 0.67 us per call at K = 1 and
 * 1.06 us at K = 4 for 65,536 sessions at 64 calls per launch; spectator emit with the unit on 1.8 % and
 * 2.7 % slower than without.  Kernel: p2p_spec_poll.hip (the step and the launch loop: poll_device.h). */
/* Part of the configuration: after ggrs_p2p_set_spectator_emit (GGRS_E_STATE without it, on a
 * fixed-latency engine and after the first call; setting spectator emit again turns the unit off),
 * disconnect_notify_start_ms > disconnect_timeout_ms is GGRS_E_INVALID. */
int ggrs_p2p_set_spectator_poll(ggrs_p2p_engine_t* eng, uint64_t disconnect_timeout_ms,
                                uint64_t disconnect_notify_start_ms, uint64_t start_ms);
/* The polls of calls first_call .. first_call + n_calls - 1, in order, each exactly once
 * (GGRS_E_INVALID otherwise, nothing launched).  now_ms [n] u64 as for ggrs_p2p_poll_endpoints: a host
 * array that decreases is GGRS_E_INVALID, a device value below the engine's last clock is taken as that
 * clock.  kinds and close_in [n][K][S] u8 (NULL: none); outputs resend (ggrs_p2p_emit_spectator_packets'
 * input), send_report and net_events [n][K][S] u8, any may be NULL.  Host arrays are staged, device
 * arrays (on_device) read and written in place on the engine's stream. */
int ggrs_p2p_poll_spectator_endpoints(ggrs_p2p_engine_t* eng, int32_t first_call, int32_t n_calls, const uint64_t* now_ms,
                                      const uint8_t* kinds, const uint8_t* close_in, uint8_t* resend,
                                      uint8_t* send_report, uint8_t* net_events, int32_t on_device);
/* Per endpoint, [K][S] each, as ggrs_p2p_read_endpoint_state.  Any pointer may be NULL. */
int ggrs_p2p_read_spectator_endpoint_state(ggrs_p2p_engine_t* eng, int32_t* state, uint64_t* last_recv_ms,
                                           uint64_t* last_input_recv_ms, uint64_t* last_report_ms,
                                           uint64_t* shutdown_ms, int32_t* flags, int32_t* closed_call);

/* ---- Event queue: every session's P2PSession::event_queue (p2p_session.rs:149) on the device, filled per
 * call from the rows the other units wrote, and P2PSession::events() (:573-576) for all sessions in one
 * call: a drain into one dense list.  Arrival-schedule mode is required; every other unit combines with
 * it, and none is required: the unit is a function of the rows it is given.  Per session a ring of
 * `capacity` 16-byte records (ggrs_event_record_t), head and length, a `closed` flag for the endpoint
 * towards the remote players (one endpoint per session holds them all, as in packet emit) and a counter
 * `dropped`, all empty / open / 0 at first.  A record: kind (GGRS_EVENT_*; no Synchronizing /
 * Synchronized kinds, which no code of the reference raises), endpoint (0: the remote players'
 * endpoint, 1 + k: spectator endpoint k -- it stands in for GgrsEvent's addr), the call that pushed it
 * and a 64-bit payload: NetworkInterrupted disconnect_timeout - disconnect_notify_start in ms
 * (protocol.rs:353-356; of ggrs_p2p_set_endpoint_poll for endpoint 0, of ggrs_p2p_set_spectator_poll for
 * the others, 0 without that unit), WaitRecommendation skip_frames, DesyncDetected frame |
 * (uint64_t)(local_checksum | remote_checksum << 16) << 32, else 0.
 * Call c, in advance_frame's order (:265-357):
 *  a. poll_remote_clients (:430-469) with handle_event (:846-902).  The remote endpoint first, in this
 *     order: GGRS_NET_RESUMED in net_events[c] pushes NetworkResumed; disc_req[c] != 0 (an accepted Input
 *     carried disconnect_requested: on_input's Event::Disconnected, protocol.rs:569-574, which the
 *     endpoint poll's rows do not hold) pushes Disconnected while the endpoint is open;
 *     GGRS_NET_INTERRUPTED pushes NetworkInterrupted; GGRS_NET_DISCONNECTED pushes Disconnected while the
 *     endpoint is open.  The endpoint closes (closed_call = c) with disc_req[c] != 0, with a remote
 *     player's bit in events[c] -- the host's own disconnect_player closes it without an event
 *     (:485-511, protocol.rs:311-319) -- and with a pushed Disconnected, in that order, so a disconnect
 *     request after the host's own disconnect and a timeout after a request raise nothing (the endpoint
 *     poll raises no GGRS_NET_DISCONNECTED for such an endpoint; the rule shows with hand-made rows
 *     only).  GGRS_NET_SHUTDOWN is no GgrsEvent.  Then spectator endpoints k = 0 .. K - 1 in ascending
 *     order (the reference walks a HashMap), K = num_spectators of ggrs_p2p_set_spectator_emit or 0:
 *     NetworkResumed, NetworkInterrupted, Disconnected from spec_net_events[c][k].  After every push, and
 *     once if handled_inputs[c] != 0 (the endpoint decoded at least one new frame: an Event::Input was
 *     handled, which pushes nothing), the oldest events go while more than 100 are queued
 *     (MAX_EVENT_QUEUE_SIZE, the end of every handle_event, :898-901);
 *  b. compare_local_checksums_against_peers (:904-937): the call's DesyncDetected records in ascending
 *     frame order, no trim;
 *  c. check_wait_recommendation (:804-817): skip_frames[c] > 0 pushes WaitRecommendation, no trim.
 * The queue may therefore hold more than 100 events between two endpoint events, as the reference's
 * does.  Stated divergences: the reference's VecDeque grows, here a push into a full ring drops the
 * oldest record and counts it in `dropped`; the rows cannot tell two reference orders apart in one case
 * -- a spectator's overflow Disconnected, queued by the previous call's send_input, against a Resumed of
 * the same poll -- and the fixed order above holds.
 * The desync records of an invocation are a list in no order; the order a session needs comes from the
 * keys (call, then frame, then the checksums).  A session takes at most 64 records from one invocation
 * (two calls' worth of the 32 reports one call can compare); with more it keeps 64 of them (which is
 * unspecified), its status becomes GGRS_EVENTS_LOST for good, and the other sessions go on.  A record
 * naming a call outside the invocation's or a session outside the engine's is passed over.
 * Out of scope: enacting a WaitRecommendation, several remote endpoints per session, fixed-latency
 * engines, peers' disconnect reports, a desync list that was full (ggrs_p2p_set_desync_compare's
 * max_events is the caller's to size).
 * Measured (profiles/event_queue_rate.json; 65,536 sessions, 64 calls per launch, a live server's event
 * density): collect 2.90 us per call at K = 0 and 4.01 us at K = 4, 3.8x and 5.3x the endpoint poll of the
 * same calls (0.76 us); a drain of one launch's 174,105 records takes 160 us of host time around the call.
 * Kernels: p2p_events.hip (the step, the collect loop and the drain: events_device.h). */
typedef struct ggrs_event_record {
  uint8_t kind;      /* GGRS_EVENT_* */
  uint8_t endpoint;  /* 0 the remote players' endpoint (a spectator's host), 1 + k spectator endpoint k */
  uint16_t reserved; /* 0 */
  int32_t call;      /* the call that pushed the record */
  uint64_t payload;
} ggrs_event_record_t;
#define GGRS_EVENT_DISCONNECTED 1
#define GGRS_EVENT_NETWORK_INTERRUPTED 2
#define GGRS_EVENT_NETWORK_RESUMED 3
#define GGRS_EVENT_WAIT_RECOMMENDATION 4
#define GGRS_EVENT_DESYNC_DETECTED 5
#define GGRS_EVENTS_LOST (-27)  /* a session had more desync records in one invocation than it can take */
/* Part of the configuration (after ggrs_p2p_set_arrival_schedule(eng, 1), before the first call):
 * capacity in 128..1024 records per session (GGRS_E_INVALID otherwise).  GGRS_E_STATE after the first
 * call and on a fixed-latency engine. */
int ggrs_p2p_set_event_queue(ggrs_p2p_engine_t* eng, int32_t capacity);
/* Steps a-c for calls first_call .. first_call + n_calls - 1: in order, each exactly once
 * (GGRS_E_INVALID otherwise, nothing launched); no ordering against ggrs_p2p_advance_frames.  Rows, any
 * may be NULL (nothing happened): events (the calls' events bytes), disc_req, handled_inputs and
 * net_events (ggrs_p2p_poll_endpoints') [n][S] u8, spec_net_events (ggrs_p2p_poll_spectator_endpoints')
 * [n][K][S] u8, skip_frames (ggrs_p2p_time_sync's) [n][S] i32.  The desync records: n_desync of them in
 * ds_call, ds_session, ds_frame, ds_local, ds_remote, as ggrs_p2p_read_desync_events returns them; or
 * n_desync == -1 with the five NULL: the engine's own list, the records ggrs_p2p_compare_reports
 * appended -- GGRS_E_STATE, naming the call, unless the comparison has run through call first_call +
 * n_calls - 1.  on_device as ggrs_p2p_emit_packets (every array then a device array, read on the
 * engine's stream).  The result does not depend on how the calls are split over invocations
 * (GGRS_EVENTS_LOST does: its bound is per invocation).  GGRS_E_STATE without ggrs_p2p_set_event_queue. */
int ggrs_p2p_collect_events(ggrs_p2p_engine_t* eng, int32_t first_call, int32_t n_calls, const uint8_t* events,
                            const uint8_t* disc_req, const uint8_t* handled_inputs, const uint8_t* net_events,
                            const uint8_t* spec_net_events, const int32_t* skip_frames, int32_t n_desync,
                            const int32_t* ds_call, const int32_t* ds_session, const int32_t* ds_frame,
                            const uint16_t* ds_local, const uint16_t* ds_remote, int32_t on_device);
/* Every session's events() at once: the queues of sessions 0, 1, .. in that order, each in queue order,
 * as one dense list -- session [max_records] i32 and records [max_records] -- and those queues left
 * empty.  With max_records too small whole sessions are drained in ascending order while they fit; the
 * first session that does not fit and all later ones keep their queues.  n_read: the records written,
 * n_left: the records still queued (host values, either may be NULL; the call waits for its launches).
 * on_device != 0: session and records are device arrays (records 16-byte aligned), written on the
 * engine's stream. */
int ggrs_p2p_drain_events(ggrs_p2p_engine_t* eng, int32_t max_records, int32_t* session, ggrs_event_record_t* records,
                          int32_t* n_read, int32_t* n_left, int32_t on_device);
/* Without draining, per session [num_sessions] i32 each: the queue's length, the records a full ring
 * dropped, the status (0, GGRS_EVENTS_LOST), the call that closed the remote endpoint (-1: open); queue
 * [capacity][num_sessions] records in queue order, zero past the length.  Any pointer may be NULL. */
int ggrs_p2p_read_event_queue_state(ggrs_p2p_engine_t* eng, int32_t* length, int32_t* dropped, int32_t* status,
                                    int32_t* closed_call, ggrs_event_record_t* queue);

/* ---------------------------------------------------------------------------------------------
 * Spectators: num_sessions independent SpectatorSessions (src/sessions/p2p_spectator_session.rs),
 * each following one host's confirmed input stream over its own network, each call =
 * SpectatorSession::advance_frame (:103-129) + the ex_game handler.  Kernel: spectator.hip.
 * Per session: current_frame and last_recv_frame start at GGRS_NULL_FRAME (:66-67), the input
 * buffer holds SPECTATOR_BUFFER_SIZE = 60 frames (:17), host_connect_status[k] = {disconnected,
 * last_frame} per player.  Call c: (1) the host's confirmed frames (last_recv, recv_upto[c]] arrive
 * (Event::Input :218-231; a value at or below what already arrived delivers nothing; the host runs on
 * its own clock, so recv_upto is not bounded by the call index); (2) the call's connect-status note
 * is merged into the host endpoint's status (UdpProtocol::on_input, src/network/protocol.rs:575-585:
 * disconnected is sticky, last_frame takes the maximum), which the session copies only with an
 * Event::Input -- at the first call at or after the note's own that delivers a new frame (:228-231);
 * (3) n = last_recv - current_frame > max_frames_behind ? catchup_speed : 1 (:109-113); (4) n times,
 * f = current_frame + 1 (inputs_at_frame :168-197): last_recv < f -> PredictionThreshold, nothing
 * advances (counted in `waited`); last_recv >= f + 60 -> SpectatorTooFarBehind, for good
 * (GGRS_E_TOO_FAR_BEHIND in the session's error; it still receives); else AdvanceFrame with input
 * row f, player k InputStatus::Disconnected (ex_game input 4) iff disconnected[k] && last_frame[k] <
 * f, and current_frame += 1.
 * catchup_speed == 1 goes with any max_frames_behind in 1..59, otherwise catchup_speed <
 * max_frames_behind (builder.rs:214-248).  Under that rule both error exits can only hit the first
 * of a call's n iterations (n > 1 means more than n frames are waiting, and last_recv < f + 60 at the
 * first iteration holds at the later ones), so the reference's dropping of already built requests
 * on `?` (:118) is never observable.
 * Per-session stops (as ggrs_p2p_add_arrivals' sessions; the others run on): a session that needs an
 * input row no longer among the input_capacity rows held when its launch started stops with
 * GGRS_E_PRECONDITION; an arrival naming a frame not yet added when its launch started stops the
 * session with GGRS_E_INVALID.  A stopped session changes no more; its calls trace 0 advances. */
typedef struct ggrs_spectator_config {
  int32_t num_sessions;      /* S >= 1 */
  int32_t num_players;       /* 1..4 (ex_game.rs:70) */
  int32_t max_frames_behind; /* 1..59 (with_max_frames_behind, builder.rs:214-229; default 10) */
  int32_t catchup_speed;     /* 1, or 2..max_frames_behind-1 (with_catchup_speed, :233-248; default 1) */
  int32_t input_capacity;    /* input rows and arrival rows held; 0 = 256; >= 64 */
  int32_t trace_capacity;    /* calls of (advanced, checksum) kept (0: none) */
  int32_t device;
} ggrs_spectator_config_t;

typedef struct ggrs_spectator_engine ggrs_spectator_engine_t;

/* host_connect_status as the host's input messages carry it (protocol.rs:575-585): `player`
 * disconnected with last frame `frame` (>= -1).  0 = no note. */
#define GGRS_SPECTATOR_NOTE(player, frame) (1 | (player) << 1 | ((frame) + 1) << 3)

/* SessionBuilder::start_spectator_session (builder.rs:310-338) with the checks of
 * with_max_frames_behind / with_catchup_speed (:214-248), SpectatorSession::new
 * (p2p_spectator_session.rs:43-71), State::new (ex_game.rs:246-269) */
int ggrs_spectator_engine_create(const ggrs_spectator_config_t* cfg, ggrs_spectator_engine_t** out);
int ggrs_spectator_engine_destroy(ggrs_spectator_engine_t* eng);
int ggrs_spectator_engine_config(const ggrs_spectator_engine_t* eng, ggrs_spectator_config_t* out);
/* The host's confirmed inputs of frames [first_frame, first_frame + n_frames), as
 * send_confirmed_inputs_to_spectators sends them (p2p_session.rs:716-745):
 * inputs [n_frames][num_sessions][num_players], added in order from frame 0.  The engine keeps the
 * newest input_capacity rows. */
int ggrs_spectator_add_inputs(ggrs_spectator_engine_t* eng, int32_t first_frame, int32_t n_frames,
                              const uint8_t* inputs);
/* recv_upto [n_calls][num_sessions] i32: the newest host frame each session's poll_remote_clients
 * (p2p_spectator_session.rs:133-156) delivered by each call; notes [n_calls][num_sessions] i32
 * (GGRS_SPECTATOR_NOTE or 0; NULL: none).  Calls in order from 0, at most input_capacity calls ahead
 * of the next call. */
int ggrs_spectator_add_arrivals(ggrs_spectator_engine_t* eng, int32_t first_call, int32_t n_calls,
                                const int32_t* recv_upto, const int32_t* notes);
/* n_calls calls of SpectatorSession::advance_frame (:103-129) + the handler for every session, one
 * launch; GGRS_E_INVALID when a call's arrival row is missing */
int ggrs_spectator_advance_frames(ggrs_spectator_engine_t* eng, int32_t n_calls);
/* advance_frame calls made */
int ggrs_spectator_calls(const ggrs_spectator_engine_t* eng, int32_t* out);
int ggrs_spectator_synchronize(ggrs_spectator_engine_t* eng);
/* per session [num_sessions] i32 each, any pointer may be NULL: SpectatorSession::current_frame
 * (:159-161), last_recv_frame (:222), the calls that returned PredictionThreshold (:175-177), and
 * the session's error: 0, GGRS_E_TOO_FAR_BEHIND (:180-182), GGRS_E_PRECONDITION or GGRS_E_INVALID */
int ggrs_spectator_read_sessions(ggrs_spectator_engine_t* eng, int32_t* current_frame, int32_t* last_recv,
                                 int32_t* waited, int32_t* errors);
/* a session's game state as bincode bytes (36 + 20 * num_players); every session's, one transfer:
 * out[num_sessions][36 + 20 * num_players] */
int ggrs_spectator_read_state(ggrs_spectator_engine_t* eng, int32_t session, uint8_t* out);
int ggrs_spectator_read_states(ggrs_spectator_engine_t* eng, uint8_t* out);
/* calls first_call .. first_call + n - 1 (run, among the last trace_capacity): advanced [n][num_sessions]
 * u8 = the AdvanceFrame requests the call returned (:120-122), checksums [n][num_sessions] u16 =
 * fletcher16 of the state after the call (ex_game.rs:121-126), whether it advanced or not.  Either
 * pointer may be NULL. */
int ggrs_spectator_read_trace(ggrs_spectator_engine_t* eng, int32_t first_call, int32_t n, uint8_t* advanced,
                              uint16_t* checksums);
int ggrs_spectator_timing_reset(ggrs_spectator_engine_t* eng);
int ggrs_spectator_timing_stop(ggrs_spectator_engine_t* eng); /* as ggrs_timing_stop */
int ggrs_spectator_timing_read(ggrs_spectator_engine_t* eng, float* total_ms, int32_t* launches);

/* ---- The spectators' packet feed (kernel: spectator_ingest.hip): a session's inputs and arrivals
 * enter as the compressed Input messages its endpoint received from the host, at the call that polled
 * them -- UdpProtocol::on_input (src/network/protocol.rs:564-642) and Event::Input
 * (p2p_spectator_session.rs:218-231) on the device.  Each session follows its host on the host's own
 * clock: the window of input rows held is per session, the input_capacity frames up to the session's
 * last received one, so the hosts of one engine may be any number of frames apart.
 * Per session, last_recv starts at GGRS_NULL_FRAME.  A packet (start, bytes) at call c, in on_input's
 * order:
 *  1. last_recv != NULL && last_recv + 1 < start is the assert! of :588-590, and so is a first packet
 *     with start != 0: the session stops at call c with GGRS_E_PRECONDITION;
 *  2. the decode reference is the blank input while last_recv == NULL, else all players' bytes of
 *     frame start - 1, the session's own row; recv_inputs keeps frames >= last_recv -
 *     2 max_prediction (:636-639): an older one drops the packet (GGRS_PACKET_NO_REFERENCE);
 *  3. compression::decode with ggrs_codec_decode's acceptance and codes; a rejected packet is dropped
 *     whole (more than max_packet_inputs inputs: GGRS_CODEC_E_CAP; a packet_len outside
 *     0..packet_stride: GGRS_CODEC_E_INVALID);
 *  4. frames <= last_recv are skipped, the later ones are stored into their rows and last_recv
 *     becomes the packet's last frame -- not bounded by the call index;
 *  5. the call's recv_upto is last_recv; its note is merged as ggrs_spectator_add_arrivals' is,
 *     whatever became of the packet (:575-585 precedes the decode).
 * A stopped session receives nothing more; its spectator stops at call c (it changes no more, its
 * calls trace 0 advances).  A SpectatorTooFarBehind session keeps receiving.  A session that must
 * advance a frame at or below last_recv - input_capacity, last_recv the feed's when the launch
 * starts -- receives were queued too far ahead of the launch for this input_capacity -- stops with
 * GGRS_E_PRECONDITION, the existing rule per session.
 *
 * Part of the configuration: before the first input, arrival and call (GGRS_E_STATE after).
 * max_prediction is the host endpoint's (builder.rs:320-329, default 8), >= 0; max_packet_inputs in
 * 1..128; packet_stride a multiple of 4, >= ggrs_codec_max_packet_bytes(num_players,
 * max_packet_inputs) and <= 1012; input_capacity > 2 * max_prediction + max_packet_inputs
 * (GGRS_E_INVALID otherwise).  From then on ggrs_spectator_add_inputs and ggrs_spectator_add_arrivals
 * return GGRS_E_STATE. */
int ggrs_spectator_set_packet_feed(ggrs_spectator_engine_t* eng, int32_t max_prediction, int32_t max_packet_inputs,
                                   int32_t packet_stride);
/* The newest packet each session's poll received by calls first_call .. first_call + n_calls - 1, in
 * call order as ggrs_spectator_add_arrivals, at most input_capacity calls ahead of the next call:
 * start_frame [n_calls][num_sessions] i32 (< 0: no packet), packet_len [n_calls][num_sessions] i32,
 * packets [n_calls][num_sessions][packet_stride] u8, one packet input = num_players bytes in player
 * order (InputBytes::from_inputs, protocol.rs:52-80); notes [n_calls][num_sessions] i32
 * (GGRS_SPECTATOR_NOTE or 0; NULL: none) -- the envelope's peer_connect_status, which ggrs_wire_unpack
 * writes as its notes.  A malformed note in host memory is GGRS_E_INVALID; with on_device the five pointers are
 * device memory (packets dword aligned) read by a launch on the engine's stream, and a malformed
 * note counts as none.  GGRS_E_STATE without ggrs_spectator_set_packet_feed. */
int ggrs_spectator_receive_packets(ggrs_spectator_engine_t* eng, int32_t first_call, int32_t n_calls,
                                   const int32_t* start_frame, const int32_t* packet_len, const uint8_t* packets,
                                   const int32_t* notes, int32_t on_device);
/* [n_calls][num_sessions] i32 each, either may be NULL, for received calls among the last
 * input_capacity: status as ggrs_p2p_read_packet_results' (1 = delivered something new, 0 = no
 * packet or nothing new, a GGRS_CODEC_* code, GGRS_PACKET_NO_REFERENCE, GGRS_PACKET_STOPPED at the
 * stopping call); ack_frame = last_recv after the call (what send_input_ack carries). */
int ggrs_spectator_read_packet_results(ggrs_spectator_engine_t* eng, int32_t first_call, int32_t n_calls,
                                       int32_t* status, int32_t* ack_frame);

/* ---- Spectator engine: endpoint poll.  SpectatorSession::poll_remote_clients
 * (p2p_spectator_session.rs:133-156) with handle_event (:199-239) over the host endpoint's
 * UdpProtocol::poll (protocol.rs:329-376, :534-551, :569-574, :608, :634), per call, on the device:
 * when to acknowledge, when a quality report is due, when the host went quiet (NetworkInterrupted /
 * NetworkResumed) and when it is gone (GgrsEvent::Disconnected).  Times, strictness and the start
 * values are "Endpoint poll"'s.  Call c at clock now = max(now_ms[c], the engine's last clock):
 *  1. kinds[c] != 0: last_recv_time = now; with disconnect_notify_sent set, the flag is cleared and
 *     GGRS_NET_RESUMED raised;
 *  2. events[c] != 0 (an accepted Input carried disconnect_requested): with disconnect_event_sent clear,
 *     GGRS_NET_DISCONNECTED is raised, the flag set and disconnected_call = c (on_input, :569-574);
 *  3. decoded = kinds has the Input bit and, with the packet feed, the feed's status of call c is >= 0:
 *     running_last_input_recv = now, send_ack[c] = 1;
 *  4. poll(), in order: (a) the retry timer resets running_last_input_recv; it has no output, because a
 *     spectator has nothing pending, and is kept so that the field equals the reference's; (b)
 *     running_last_quality_report + 200 < now: send_report[c] = 1, the time set; (c)
 *     GGRS_NET_INTERRUPTED as in "Endpoint poll"; (d) disconnect_event_sent clear and last_recv_time +
 *     disconnect_timeout < now: GGRS_NET_DISCONNECTED, the flag set, disconnected_call = c.
 * Where this differs from the P2P units: the reference's spectator never calls host.disconnect() --
 * handle_event only forwards the event -- so the endpoint stays Running for good, its timers and the
 * interrupted / resumed pair go on after the one Disconnected, and GGRS_NET_SHUTDOWN never appears.
 * GGRS_NET_DISCONNECTED stands for both causes here (the spectator engine has no events row in which
 * the requested one could be seen).  The poll changes nothing in the sessions: a spectator whose host is
 * gone waits, as the reference's does.  No keep-alive row (see "Endpoint poll").  Out of scope:
 * NetworkStats, the spectator's update_local_frame_advantage (protocol.rs:260-269:
 * the report's frame_advantage stays the caller's input to ggrs_wire_pack), enacting anything on the
 * sessions (the GgrsEvent queue with MAX_EVENT_QUEUE_SIZE is "Spectator engine: event queue" below).
 * Measured (profiles/spectator_poll_rate.json): 0.65 us per call for 65,536 sessions at 64
 * calls per launch.  Kernel: spectator_poll.hip (the step and the launch loop: poll_device.h). */
/* Part of the configuration: GGRS_E_STATE after the first call or arrival;
 * disconnect_notify_start_ms > disconnect_timeout_ms is GGRS_E_INVALID. */
int ggrs_spectator_set_endpoint_poll(ggrs_spectator_engine_t* eng, uint64_t disconnect_timeout_ms,
                                     uint64_t disconnect_notify_start_ms, uint64_t start_ms);
/* The polls of calls first_call .. first_call + n_calls - 1: in call order, each exactly once; with the
 * packet feed after the call's packets were received and while its status row is among the
 * input_capacity rows held (GGRS_E_INVALID otherwise, nothing launched).  No ordering against
 * ggrs_spectator_advance_frames.  now_ms [n] u64: a host array that decreases is GGRS_E_INVALID, a
 * device value below the engine's last clock is taken as that clock.  kinds and events [n][S] u8 as
 * ggrs_wire_unpack writes them (NULL: none); outputs send_ack, send_report (ggrs_wire_pack's) and
 * net_events (GGRS_NET_* bits) [n][S] u8, any may be NULL.  Host arrays are staged, device arrays
 * (on_device) read and written in place on the engine's stream.  The result does not depend on how the
 * calls are split over invocations. */
int ggrs_spectator_poll_endpoints(ggrs_spectator_engine_t* eng, int32_t first_call, int32_t n_calls,
                                  const uint64_t* now_ms, const uint8_t* kinds, const uint8_t* events, uint8_t* send_ack,
                                  uint8_t* send_report, uint8_t* net_events, int32_t on_device);
/* Per session, [num_sessions] each: the three times, flags (bit 0 disconnect_notify_sent, bit 1
 * disconnect_event_sent) and the call that raised the one Disconnected (-1).  Any pointer may be NULL. */
int ggrs_spectator_read_endpoint_state(ggrs_spectator_engine_t* eng, uint64_t* last_recv_ms, uint64_t* last_input_recv_ms,
                                       uint64_t* last_report_ms, int32_t* flags, int32_t* disconnected_call);

/* ---- Spectator engine: event queue.  SpectatorSession::handle_event (p2p_spectator_session.rs:199-239)
 * over the endpoint poll's net_events row, kept per session on the device, and events() for all
 * sessions in one call.  Step a of "Event queue" alone, for the session's one host endpoint (endpoint 0):
 * NetworkResumed, NetworkInterrupted (payload: ggrs_spectator_set_endpoint_poll's disconnect_timeout -
 * disconnect_notify_start, 0 without it), Disconnected -- GGRS_NET_DISCONNECTED already stands for both
 * causes here, and it is pushed once (closed_call).  Every push and every handled Input
 * (handled_inputs[c] != 0) trims, so a queue never holds more than 100 events; status stays 0.  The
 * ring, `dropped`, the drain and the read-back are the P2P unit's; its own speed has not been
 * measured (the collect loop is the P2P unit's without its second half).  Kernels: spectator_events.hip (events_device.h). */
/* Part of the configuration: GGRS_E_STATE after the first call or arrival; capacity in 128..1024
 * (GGRS_E_INVALID otherwise). */
int ggrs_spectator_set_event_queue(ggrs_spectator_engine_t* eng, int32_t capacity);
/* Calls first_call .. first_call + n_calls - 1, in order, each exactly once (GGRS_E_INVALID otherwise,
 * nothing launched): handled_inputs and net_events [n][S] u8, either may be NULL.  on_device: device
 * arrays, read on the engine's stream.  The result does not depend on how the calls are split. */
int ggrs_spectator_collect_events(ggrs_spectator_engine_t* eng, int32_t first_call, int32_t n_calls,
                                  const uint8_t* handled_inputs, const uint8_t* net_events, int32_t on_device);
/* As ggrs_p2p_drain_events and ggrs_p2p_read_event_queue_state. */
int ggrs_spectator_drain_events(ggrs_spectator_engine_t* eng, int32_t max_records, int32_t* session,
                                ggrs_event_record_t* records, int32_t* n_read, int32_t* n_left, int32_t on_device);
int ggrs_spectator_read_event_queue_state(ggrs_spectator_engine_t* eng, int32_t* length, int32_t* dropped,
                                          int32_t* status, int32_t* closed_call, ggrs_event_record_t* queue);

/* ---- Input wire codec, batched (src/network/compression.rs:14-182; bitfield-rle 0.2.1 runs,
 * bincode 1.3 fixint framing of EncodedInputSequence).  Replaces compression::encode / decode as
 * called per endpoint by UdpProtocol::send_pending_output (protocol.rs:450-480) and on_input
 * (:580-642), for many packets per launch: one packet = a reference input and the pending inputs
 * encoded against it, every input input_bytes long (what a GGRS peer sends for a fixed-size
 * Config::Input).  All pointers are DEVICE pointers; `stream` is a hipStream_t (NULL: default).
 * Per-packet results are written to device memory (asynchronous with the host). */
#define GGRS_CODEC_OK 0
#define GGRS_CODEC_E_BINCODE -1   /* bincode::deserialize failed (bad tag, short buffer) */
#define GGRS_CODEC_E_RLE -2       /* bitfield_rle::decode failed (truncated header or literal) */
#define GGRS_CODEC_E_DELTA -3     /* delta_decode rejected the sizes (compression.rs:117-154) */
#define GGRS_CODEC_E_CAP -4       /* encode: out_stride too small; decode: more than max_inputs */
#define GGRS_CODEC_E_INVALID -5   /* count outside 0..max_inputs, length outside 0..stride */
#define GGRS_CODEC_UNSUPPORTED -6 /* valid packet whose inputs are not all input_bytes long */
/* encode: ref [n][input_bytes], pending [n][max_inputs][input_bytes], count [n] ->
 * out [n][out_stride] packet bytes, out_len [n] = packet length or a GGRS_CODEC_E_* code */
int ggrs_codec_encode(const uint8_t* ref, const uint8_t* pending, const int32_t* count, int64_t n_packets,
                      int32_t input_bytes, int32_t max_inputs, uint8_t* out, int32_t out_stride, int32_t* out_len,
                      void* stream);
/* decode: ref [n][input_bytes], packets [n][packet_stride] with packet_len [n] bytes ->
 * out [n][max_inputs][input_bytes], count [n], status [n] (GGRS_CODEC_OK or an error code;
 * never faults on hostile bytes -- decode_arbitrary_input_never_panics, compression.rs:205-213).
 * Every row of out is written whole: the slots past count, and a failed packet's row, are zero
 * (out needs no clearing beforehand). */
int ggrs_codec_decode(const uint8_t* ref, const uint8_t* packets, const int32_t* packet_len, int64_t n_packets,
                      int32_t packet_stride, int32_t input_bytes, int32_t max_inputs, uint8_t* out, int32_t* count,
                      int32_t* status, void* stream);
/* The same with the chunked packet layout: the packets of each block of 256 (packets
 * 256 b .. 256 b + 255) lie back to back from byte 256 * b * stride of out / packets, each padded to
 * a multiple of 4 bytes; a packet whose length is outside [1, stride] (an error code) takes no
 * bytes.  Packet i's offset is 256 * (i / 256) * stride plus the padded lengths of the block's
 * packets before it, so the lengths alone locate every packet; the kernels move exactly the
 * packets' bytes instead of whole stride-byte rows.  Requires input_bytes in {1, 2, 4},
 * max_inputs * input_bytes <= 64 and a multiple of 4, stride a multiple of 4, dword-aligned
 * buffers (GGRS_E_INVALID otherwise). */
int ggrs_codec_encode_chunked(const uint8_t* ref, const uint8_t* pending, const int32_t* count, int64_t n_packets,
                              int32_t input_bytes, int32_t max_inputs, uint8_t* out, int32_t out_stride,
                              int32_t* out_len, void* stream);
int ggrs_codec_decode_chunked(const uint8_t* ref, const uint8_t* packets, const int32_t* packet_len, int64_t n_packets,
                              int32_t packet_stride, int32_t input_bytes, int32_t max_inputs, uint8_t* out,
                              int32_t* count, int32_t* status, void* stream);
/* an out_stride that every packet of max_inputs inputs fits (a multiple of 16) */
int32_t ggrs_codec_max_packet_bytes(int32_t input_bytes, int32_t max_inputs);
/* kernel forms (for tests and comparison; process-wide): 0 = default (lane-cooperative where
 * max_inputs * input_bytes <= 64 and rows are whole dwords, else thread-per-packet LDS-staged where
 * rows are whole dwords, else direct), 1 = direct thread-per-packet, 2 = thread-per-packet
 * LDS-staged where it applies */
int ggrs_codec_set_direct(int32_t mode);

/* ---- Wire envelope, batched (kernel: wire.hip): what a socket hands a GGRS host is a datagram,
 * bincode::serialize(&Message) (src/network/udp_socket.rs, src/network/messages.rs:5-129).  Unpack turns
 * the raw datagrams of a poll into the dense arrays the P2P and spectator units take -- UdpProtocol::
 * handle_message (src/network/protocol.rs:534-562), on_input's envelope part (:564-585), on_input_ack,
 * on_quality_report and on_quality_reply (:644-660) -- and pack turns the units' output arrays into
 * datagrams (queue_message :515-528 over the bodies of :450-513 and :692-698), so two engines play each
 * other datagram to datagram in the bytes a GGRS 0.10.2 peer sends and accepts.  Stateless like the
 * codec: all pointers are DEVICE pointers, `stream` is a hipStream_t (NULL: default).
 * Layout (bincode 1.3: fixed-width little-endian integers, u32 enum tag, u64 Vec length, a bool as one
 * byte that must be 0 or 1, u128 as 16 bytes, declaration order, trailing bytes accepted):
 *   Message            = magic u16 | tag u32 | body
 *   Input (0)          = n u64 | n x (disconnected u8, last_frame i32) | disconnect_requested u8
 *                        | start_frame i32 | ack_frame i32 | len u64 | bytes[len]   (31 + 5 n + len bytes)
 *   InputAck (1)       = ack_frame i32                                            (10)
 *   QualityReport (2)  = frame_advantage i16 | ping u128                          (24)
 *   QualityReply (3)   = pong u128                                                (22)
 *   ChecksumReport (4) = checksum u128 | frame i32                                (26)
 *   KeepAlive (5)      = nothing                                                  (6)
 * handle_message never checks the magic (0.10.2 has no sync handshake): unpack ignores it, pack writes
 * the endpoint's.  What stays with the host: the sockets and NetworkStats' send_queue_len and kbps_sent.
 * The 200 ms timers (which calls set resend, send_ack and send_report), NetworkInterrupted /
 * NetworkResumed and the disconnect timeouts are ggrs_p2p_poll_endpoints' (above; it also states why
 * keep_alive is never due). */
#define GGRS_WIRE_INPUT 0
#define GGRS_WIRE_INPUT_ACK 1
#define GGRS_WIRE_QUALITY_REPORT 2
#define GGRS_WIRE_QUALITY_REPLY 3
#define GGRS_WIRE_CHECKSUM_REPORT 4
#define GGRS_WIRE_KEEP_ALIVE 5
/* slot_status: tag + 1 (1..6) = accepted, 0 = empty slot, else why the datagram was dropped whole: */
#define GGRS_WIRE_E_BINCODE (-22) /* bincode::deserialize fails: short buffer, tag > 5, a bool byte > 1, a Vec
                                     length that does not fit the datagram, a length beyond dgram_stride */
#define GGRS_WIRE_E_SHAPE (-23)   /* an Input with fewer than num_statuses connect statuses: the reference indexes
                                     past the end and panics (:577-578); extra entries are ignored as it ignores them */
#define GGRS_WIRE_E_CAP (-24)     /* an Input whose bytes are longer than packet_stride */
#define GGRS_WIRE_E_CLOCK (-25)   /* a QualityReply whose pong exceeds now_ms or has any of its upper 64 bits set:
                                     the reference's assert! (:658) */
#define GGRS_WIRE_E_RANGE (-26)   /* a ChecksumReport whose checksum does not fit the engine's 16 bits (a peer
                                     running this game sends Fletcher-16 widened to u128): stated divergence,
                                     counted, never silently truncated */
/* 31 + 5 num_statuses + body_bytes rounded up to a multiple of 16: a dgram_stride every Input message of
 * num_statuses statuses and body_bytes bytes fits */
int32_t ggrs_wire_max_datagram_bytes(int32_t num_statuses, int32_t body_bytes);
/* n_calls polls of num_sessions (S) endpoints, `slots` (M, 1..8) datagram slots per poll; num_statuses
 * 1..4 (the session's players); remote_mask the events bits a disconnect request sets; first_call >= 0
 * the call of row 0 (it rotates notes).  Inputs: dgrams [n][M][S][dgram_stride] u8 (dword aligned,
 * dgram_stride a multiple of 4 in 8..2048), dgram_len [n][M][S] i32 (<= 0: empty; > dgram_stride:
 * GGRS_WIRE_E_BINCODE), now_ms [n] u64 (the host's millis_since_epoch at each poll); packet_stride a
 * multiple of 4 in 4..1012.  Outputs, [n][S] unless noted, any may be NULL; the slots of one (call,
 * session) are folded in slot order, as handle_message would be called on them, a dropped datagram
 * changing nothing:
 *   slot_status [n][M][S] i32;
 *   start_frame i32, packet_len i32, packets [n][S][packet_stride] u8 (dword aligned): the arrays
 *     ggrs_p2p_receive_packets and ggrs_spectator_receive_packets read, holding the accepted Input with
 *     the greatest start_frame, ties to the later slot; -1 / 0 without one.  A sender's start_frame is
 *     its first unacknowledged frame, which never decreases, and it learned start_frame - 1 from an ack
 *     this receiver sent, so that packet alone delivers every frame the fold over all of them would.
 *     Stated divergence: two equal-start_frame packets arriving in reversed order lose the longer one's
 *     tail until the next resend.  Bytes past packet_len are unspecified;
 *   ack_in i32: the maximum of every accepted Input's and InputAck's ack_frame (pop_pending_output is
 *     monotone, so the maximum equals the fold), GGRS_NULL_FRAME without one;
 *   events u8: remote_mask when an accepted Input has disconnect_requested, else 0;
 *   disc_mask u8 and last_frame [n][num_statuses][S] i32: the sticky merge of :577-584 over the poll's
 *     accepted Inputs with disconnect_requested == false (bits 0, last_frame GGRS_NULL_FRAME without
 *     one); the host keeps merging across polls, or feeds ggrs_p2p_add_peer_reports from it;
 *   notes i32: the same status as ggrs_spectator_receive_packets takes it: 0 when no bit is set, else
 *     with m set bits GGRS_SPECTATOR_NOTE(player, last_frame) of the ((first_call + i) mod m)-th in
 *     ascending player order, the rule of ggrs_p2p_emit_spectator_packets' notes;
 *   remote_advantage i32: the last accepted QualityReport's frame_advantage, sign-extended, else
 *     GGRS_TIME_SYNC_KEEP; ping [n][S][16] u8 (dword aligned): that report's ping, verbatim, for the
 *     reply (zeros without one).  Stated divergence: several reports of one poll get one reply, to the last;
 *   rtt_ms i32: now_ms[i] - pong of the last accepted QualityReply, saturated at INT32_MAX
 *     (ggrs_p2p_time_sync clamps further), -1 without one;
 *   report_frame i32 and report_checksum u16: the accepted ChecksumReport with the greatest frame (ties
 *     to the later slot), else GGRS_NULL_FRAME and 0.  Stated divergence: a poll keeps one report, the
 *     older ones of a burst are dropped (their slot_status still counts them);
 *   kinds u8: bit t set when a message of tag t was accepted.
 * Never faults on hostile bytes; every output of a (call, session) is written whole, whatever the
 * datagrams hold.  Bad arguments: GGRS_E_INVALID, nothing launched. */
int ggrs_wire_unpack(int32_t n_calls, int32_t num_sessions, int32_t slots, int32_t num_statuses, uint32_t remote_mask,
                     int32_t first_call, const uint8_t* dgrams, int32_t dgram_stride, const int32_t* dgram_len,
                     const uint64_t* now_ms, int32_t packet_stride, int32_t* slot_status, int32_t* start_frame,
                     int32_t* packet_len, uint8_t* packets, int32_t* ack_in, uint8_t* events, uint8_t* disc_mask,
                     int32_t* last_frame, int32_t* notes, int32_t* remote_advantage, uint8_t* ping, int32_t* rtt_ms,
                     int32_t* report_frame, uint16_t* report_checksum, uint8_t* kinds, void* stream);
/* The units' output arrays of n_calls calls -> dgrams [n][4][S][dgram_stride] and dgram_len [n][4][S]:
 * unpack's input layout with M = 4, so one engine's output is its peer's input through index arithmetic
 * alone.  magic [S] u16 and now_ms [n] u64 are required; every other input is [n][S] unless noted and
 * may be NULL (absent): start_frame, packet_len, ack_frame, packets [n][S][packet_stride] as
 * ggrs_p2p_emit_packets writes them; disc_mask u8, last_frame [n][num_statuses][S] and
 * disconnect_requested u8 for the Input envelope (absent: connected, GGRS_NULL_FRAME, false); send_ack
 * u8; send_report u8 and local_advantage of ggrs_p2p_time_sync; kinds u8 and ping [n][S][16] as unpack
 * wrote them; report_frame and report_checksum u16; keep_alive u8.  Fixed slots, an empty one has
 * length 0:
 *   0  Input{num_statuses statuses, disconnect_requested, start_frame, ack_frame, the packet's bytes} when
 *      start_frame, packet_len and packets are present, start_frame >= 0 and 0 < packet_len <=
 *      packet_stride; else InputAck{ack_frame} when send_ack; else KeepAlive when keep_alive and slots
 *      1-3 are empty too (an absent ack_frame is GGRS_NULL_FRAME);
 *   1  QualityReport{local_advantage clamped to i16, ping = now_ms} when send_report;
 *   2  QualityReply{pong = ping} when kinds has the QualityReport bit;
 *   3  ChecksumReport{checksum as u128, frame} when report_frame >= 0.
 * dgram_stride: a multiple of 4, >= ggrs_wire_max_datagram_bytes(num_statuses, packet_stride), <= 2048
 * (GGRS_E_INVALID otherwise, nothing launched).  Bytes past a datagram's length are unspecified.
 * Routing checksum reports to the compare unit: a report unpacked at poll c goes into
 * ggrs_p2p_add_remote_reports row c - 1 with local_last = GGRS_NULL_FRAME; ggrs_p2p_compare_reports(c)
 * then delivers it in call c, where the reference's poll_remote_clients would. */
int ggrs_wire_pack(int32_t n_calls, int32_t num_sessions, int32_t num_statuses, const uint16_t* magic,
                   const uint64_t* now_ms, const int32_t* start_frame, const int32_t* packet_len,
                   const int32_t* ack_frame, const uint8_t* packets, int32_t packet_stride, const uint8_t* disc_mask,
                   const int32_t* last_frame, const uint8_t* disconnect_requested, const uint8_t* send_ack,
                   const uint8_t* send_report, const int32_t* local_advantage, const uint8_t* kinds, const uint8_t* ping,
                   const int32_t* report_frame, const uint16_t* report_checksum, const uint8_t* keep_alive,
                   uint8_t* dgrams, int32_t dgram_stride, int32_t* dgram_len, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* GGRS_AMD_H */
