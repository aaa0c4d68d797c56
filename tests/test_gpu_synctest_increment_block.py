"""GPU parity of the check_distance-8, two-player SyncTest kernel whose block pass publishes each
core step's velocity increment (ggrs_amd/csrc/synctest_sincos_block.h, increment_block_pass): the
lane that evaluates the sin/cos of the rot step u + 1 starts from folds it with its own record of
that step's row, and a core step adds the 8-byte entry instead of deriving the increment from the
sin/cos and its record.

Bit-exact against the oracle's SyncTestSession, every lane: the per-frame display checksums, the
final state, and the saved-state ring's frames, checksums and state bytes (check_lane of
test_gpu_synctest); status all zero.  R = max_prediction + 1 = 10 and 16, input delay 0 and 2, on one
full block (4 lanes) and a full block plus a one-session block (5 lanes).

A session's first cd + 1 calls have no rollback yet and always run on the sequential kernel, so every
case first advances cd + 1 frames in a call of its own (see test_gpu_synctest_save_once.py); each
listed launch is then exactly one launch of the batched kernel.

Inputs: an increment depends on the row's thrust / brake / neither and on the rot the step starts
from, so the models change both from frame to frame: an entry folded with a neighbouring row's
record, or read from another player's lane, gives another velocity.
"""
import numpy as np
import pytest

from tests.test_gpu_synctest import check_lane, lane_inputs, make_engine, run_chunks

pytestmark = pytest.mark.gpu

CD, PLAYERS = 8, 2
UP, DOWN, LEFT, RIGHT = 1, 2, 4, 8

LAUNCHES = [
    [16],          # one core block between the edge blocks: step 0's increment folded in front of the loop
    [24],          # two core blocks: role 7's entry carried into the second, both entry buffers
    [16, 16, 16],  # the sin/cos re-evaluated behind a launch's last core block feeds the next launch
    [176],         # every quadrant of a held turn inside core blocks
    [544],         # role 7's record of row t + 8 across the re-read of the raw input rows
]


def turn_thrust_brake(lanes, frames):
    """a held turn (its direction per player and lane) with thrust and brake alternating every frame,
    out of phase per player and lane"""
    f = np.arange(frames)[:, None, None] + np.arange(lanes)[None, :, None] + np.arange(PLAYERS)[None, None, :]
    turn = np.where((np.arange(lanes)[:, None] + np.arange(PLAYERS)[None, :]) & 1, LEFT, RIGHT)[None]
    return (np.where(f & 1, UP, DOWN) | turn).astype(np.uint8)


def thrust_every_third(lanes, frames):
    """thrust every third frame, out of phase per player and lane, with turns alternating every frame"""
    f = np.arange(frames)[:, None, None] + np.arange(lanes)[None, :, None] + 2 * np.arange(PLAYERS)[None, None, :]
    return (np.where(f % 3 == 0, UP, 0) | np.where(f & 1, LEFT, RIGHT)).astype(np.uint8)


def thrust_and_turn(lanes, frames):
    """thrust with a held turn: the terminal speed 12.5 is above the cap of 7, so the speed clamp fires
    in every core block once the ship is up to speed; the turn's direction differs per player and lane"""
    inp = np.zeros((frames, lanes, PLAYERS), np.uint8)
    turn = np.where((np.arange(lanes)[:, None] + np.arange(PLAYERS)[None, :]) & 1, LEFT, RIGHT)
    inp[:] = (UP | turn).astype(np.uint8)[None]
    return inp


def held_keys(oracle, seed):
    return lambda lanes, frames: lane_inputs(oracle, seed, lanes, frames, PLAYERS, 0)


MODELS = ["turn_thrust_brake", "thrust_every_third", "thrust_and_turn", "held_keys"]


@pytest.mark.parametrize("delay", [0, 2])
@pytest.mark.parametrize("maxp", [9, 15])
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("launches", LAUNCHES, ids=["_".join(map(str, n)) for n in LAUNCHES])
@pytest.mark.parametrize("lanes", [4, 5])
def test_block_increment_every_lane(oracle, lanes, launches, model, maxp, delay):
    frames = CD + 1 + sum(launches)
    gen = {"turn_thrust_brake": turn_thrust_brake, "thrust_every_third": thrust_every_third,
           "thrust_and_turn": thrust_and_turn, "held_keys": held_keys(oracle, 9100 + 16 * lanes + maxp + delay)}[model]
    inputs = np.ascontiguousarray(gen(lanes, frames))
    assert inputs.shape == (frames, lanes, PLAYERS)
    eng = make_engine(lanes, PLAYERS, maxp, CD, delay, frames)
    assert run_chunks(eng, inputs, [CD + 1] + launches) == frames
    assert eng.current_frame() == frames
    trace = eng.trace(0, frames)
    for lane in range(lanes):
        check_lane(oracle, eng, inputs, lane, PLAYERS, maxp, CD, delay, frames, trace)
    status, _, _ = eng.mismatches()
    assert (status == 0).all()
