"""GPU parity of the check_distance-8, two-player SyncTest kernel whose producer wave runs a core
block's eight turns and one sin/cos evaluation per lane at the block's head
(ggrs_amd/csrc/synctest_sincos_block.h) instead of one evaluation inside every step.

Bit-exact against the oracle's SyncTestSession, every lane: the per-frame display checksums, the
final state, and the saved-state ring's frames, checksums and state bytes (check_lane of
test_gpu_synctest); status all zero.  R = max_prediction + 1 = 10 and 16, input delay 0 and 2, on one
full block (4 lanes) and a full block plus a one-session block (5 lanes).

A session's first cd + 1 calls have no rollback yet and always run on the sequential kernel, so every
case first advances cd + 1 frames in a call of its own (see test_gpu_synctest_save_once.py); each
listed launch is then exactly one launch of the batched kernel.

Inputs: the turn is what the block's rotation chain and its entries depend on, so three of the four
models hold or alternate turns on both players; at 2.5 / 60 rad per frame a held turn wraps after
151 frames, so the 176- and 544-frame launches wrap inside core blocks, in both directions (player 0
left: below 0; player 1 right: at 2 pi).
"""
import numpy as np
import pytest

from tests.test_gpu_synctest import check_lane, lane_inputs, make_engine, run_chunks

pytestmark = pytest.mark.gpu

CD, PLAYERS = 8, 2
UP, DOWN, LEFT, RIGHT = 1, 2, 4, 8

LAUNCHES = [
    [16],          # one core block between the edge blocks
    [24],          # two core blocks: both hand-off and both entry buffers
    [48, 40],      # every ring slot at every block position (R = 10)
    [16, 16, 16],  # the rot and sin/cos a launch leaves are the next launch's
    [176],         # more than one revolution of a held turn: both wraps inside core blocks
    [544],         # crosses the re-read of the raw input rows, with records read ahead
]


def held_turns(lanes, frames):
    """player 0 holds left, player 1 holds right"""
    inp = np.zeros((frames, lanes, PLAYERS), np.uint8)
    inp[:, :, 0], inp[:, :, 1] = LEFT, RIGHT
    return inp


def alternating_turns(lanes, frames):
    """both players alternate left and right every frame, out of phase with each other and from lane to lane"""
    f = np.arange(frames)[:, None, None] + np.arange(lanes)[None, :, None] + np.arange(PLAYERS)[None, None, :]
    return np.where(f & 1, LEFT, RIGHT).astype(np.uint8)


def thrust_and_turn(lanes, frames):
    """thrust with a held turn: the terminal speed 12.5 is above the cap of 7, so the speed clamp fires
    in every core block once the ship is up to speed; the turn's direction differs per player and lane"""
    inp = np.zeros((frames, lanes, PLAYERS), np.uint8)
    turn = np.where((np.arange(lanes)[:, None] + np.arange(PLAYERS)[None, :]) & 1, LEFT, RIGHT)
    inp[:] = (UP | turn).astype(np.uint8)[None]
    return inp


def held_keys(oracle, seed):
    return lambda lanes, frames: lane_inputs(oracle, seed, lanes, frames, PLAYERS, 0)


MODELS = ["held_turns", "alternating_turns", "thrust_and_turn", "held_keys"]


@pytest.mark.parametrize("delay", [0, 2])
@pytest.mark.parametrize("maxp", [9, 15])
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("launches", LAUNCHES, ids=["_".join(map(str, n)) for n in LAUNCHES])
@pytest.mark.parametrize("lanes", [4, 5])
def test_block_sincos_every_lane(oracle, lanes, launches, model, maxp, delay):
    frames = CD + 1 + sum(launches)
    gen = {"held_turns": held_turns, "alternating_turns": alternating_turns, "thrust_and_turn": thrust_and_turn,
           "held_keys": held_keys(oracle, 7300 + 16 * lanes + maxp + delay)}[model]
    inputs = np.ascontiguousarray(gen(lanes, frames))
    eng = make_engine(lanes, PLAYERS, maxp, CD, delay, frames)
    assert run_chunks(eng, inputs, [CD + 1] + launches) == frames
    assert eng.current_frame() == frames
    trace = eng.trace(0, frames)
    for lane in range(lanes):
        check_lane(oracle, eng, inputs, lane, PLAYERS, maxp, CD, delay, frames, trace)
    status, _, _ = eng.mismatches()
    assert (status == 0).all()
