"""Arrival schedules that take a remote InputQueue to its 128 entries (input_queue.rs:6), shared by
tests/test_input_queue_model.py (CPU) and tests/test_gpu_p2p_queue_bound.py.  A helper, not a test
file.  Every schedule is one session's arrive column: the newest remote frame each call's poll
delivers, non-decreasing, at most the call.  A rung's own part is its first LADDER_CALLS /
RATE_CALLS calls; in a longer table nothing more arrives after it (the session waits: no input is
added, so it cannot overflow later)."""
import numpy as np

LADDER_CALLS, RATE_CALLS, JITTER_CALLS = 180, 320, 300
STALLS = tuple(range(100, 150))
LAGS = (1, 2, 3, 4, 5)
CATCH_UP = tuple(range(121, 141))
RATE_HOLDS = tuple(range(230, 260))


def _held(a, own, calls):
    out = np.empty(calls, np.int64)
    out[:own] = a[:own]
    out[own:] = a[own - 1]
    return np.maximum.accumulate(np.maximum(out, -1)).astype(np.int32)


def stall(L, calls=LADDER_CALLS, at=20):
    """Remote inputs one call late, nothing for L calls from call `at`, then one call late again: the
    burst after the silence is L + 1 frames."""
    a = np.arange(LADDER_CALLS) - 1
    a[at:at + L] = a[at - 1]
    return _held(a, LADDER_CALLS, calls)


def rate(lag, calls=RATE_CALLS):
    """Remote inputs `lag` calls late throughout.  A lockstep session at input delay 0 advances every
    other call, so its remote queue grows by a frame every two calls."""
    return _held(np.arange(RATE_CALLS) - lag, RATE_CALLS, calls)


def rate_hold(v, calls=RATE_CALLS):
    """Remote inputs one call late up to call v - 1, then nothing: a lockstep session at input delay 0
    comes within a few entries of the bound (it would stop at call 253) and then catches up."""
    a = np.arange(RATE_CALLS) - 1
    a[v:] = a[v - 1]
    return _held(a, RATE_CALLS, calls)


def catch_up(u, calls=LADDER_CALLS, silent=140, first=120, lag=9):
    """Nothing for `silent` calls, frames 0 .. first at call `silent`, frames up to u at the next call,
    then `lag` calls late: a session whose current frame is far behind its calls, so that the remote
    inputs run ahead of it without one long burst (and, where it survives call silent + 1, stay
    about silent - lag frames ahead of it to the end)."""
    a = np.arange(LADDER_CALLS) - lag
    a[:silent] = -1
    a[silent] = first
    a[silent + 1] = u
    return _held(a, LADDER_CALLS, calls)


def silent_start(burst, calls):
    """Nothing until one burst of `burst` frames (frames 0 .. burst - 1) at call `burst`, then one call
    late."""
    a = np.arange(calls) - 1
    a[:burst] = -1
    a[burst] = burst - 1
    return _held(a, calls, calls)


RUNGS = ([("stall", L) for L in STALLS] + [("rate", lag) for lag in LAGS] + [("catch_up", u) for u in CATCH_UP] +
         [("rate_hold", v) for v in RATE_HOLDS])
_BUILD = dict(stall=stall, rate=rate, catch_up=catch_up, rate_hold=rate_hold)


def rung_table(S, calls=RATE_CALLS, rungs=RUNGS):
    """arrive [calls][S] and the rung (kind, value) of each session: `rungs` in turn."""
    labels = [rungs[s % len(rungs)] for s in range(S)]
    return np.stack([_BUILD[k](v, calls) for k, v in labels], axis=1), labels
