"""GPU parity of the spectator engine's event queue (ggrs_spectator_set_event_queue / collect_events /
drain_events / read_event_queue_state, csrc/spectator_events.hip and events_device.h) against
tests/event_queue_model.py at S = 130: the trim, a split of the calls, the drain, misuse."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")  # loads torch's HIP runtime before the engine library

from tests import event_queue_cases as C  # noqa: E402
from tests import event_queue_model as M  # noqa: E402
from tests.test_gpu_event_queue import assert_drained, assert_matches  # noqa: E402

pytestmark = pytest.mark.gpu


def engine(queue=True, capacity=C.CAPACITY):
    from ggrs_amd import SpectatorEngine
    e = SpectatorEngine(C.S, num_players=2, input_capacity=64)
    e.set_endpoint_poll(2000, 500, 0)  # (the NetworkInterrupted payload: 1500 ms)
    if queue:
        e.set_event_queue(capacity)
    return e


def drive(eng, case, pieces, device=False):
    for i, (c0, n) in enumerate(C.pieces_of(pieces, case["calls"])):
        rows = [case["handled"][c0:c0 + n], case["net"][c0:c0 + n]]
        on_device = device is True or (device == "both" and i % 2 == 0)
        if on_device:
            rows = [torch.from_numpy(np.ascontiguousarray(r)).cuda() for r in rows]
        eng.collect_events(c0, n, *rows, on_device=on_device)
        if on_device:
            eng.synchronize()


def test_the_trim_whatever_the_split_and_the_drain():
    case = C.spectator_case()
    m = C.run_model(case, spectator=True)
    length, dropped, status, closed = C.words(m)
    assert length.max() == M.MAX_EVENT_QUEUE_SIZE and (length == 100).sum() > 10 and (length < 20).any()
    assert (dropped == 0).all() and (status == 0).all() and (closed >= 0).any() and (closed < 0).any()
    split, whole = engine(), engine()
    drive(split, case, C.PIECES, "both")
    drive(whole, case, (case["calls"],))
    assert_matches(split, m)
    assert_matches(whole, m)
    # a drain one short of a session boundary, then the rest
    ends = np.cumsum(length)
    got, left = whole.drain_events(int(ends[40]) - 1)
    want, want_left = m.drain(int(ends[40]) - 1)
    assert left == want_left > 0 and len(want) == ends[39]
    assert_drained(got, want)
    assert_matches(whole, m)
    got, left = whole.drain_events()
    want, _ = m.drain(10 ** 6)
    assert left == 0
    assert_drained(got, want)
    # ... and the queues go on after it
    whole.collect_events(case["calls"], 1, net_events=np.full((1, C.S), M.NET_RESUMED, np.uint8))
    m.collect(case["calls"], 1, net=np.full((1, C.S), M.NET_RESUMED, np.uint8))
    assert_matches(whole, m)


def test_misuse():
    from ggrs_amd._lib import GGRS_E_STATE, GgrsError, InvalidRequest
    case = C.spectator_case()

    def state_error(fn):
        with pytest.raises(GgrsError) as e:
            fn()
        assert e.value.code == GGRS_E_STATE, e.value

    plain = engine(queue=False)
    state_error(lambda: plain.collect_events(0, 1))                    # unconfigured
    state_error(plain.drain_events)
    state_error(plain.event_queue_state)
    for capacity in (127, 1025):
        with pytest.raises(InvalidRequest):
            plain.set_event_queue(capacity)
    plain.add_inputs(0, np.zeros((1, C.S, 2), np.uint8))
    plain.add_arrivals(0, np.zeros((1, C.S), np.int32))
    state_error(lambda: plain.set_event_queue(128))                    # after the first arrival
    eng = engine()
    with pytest.raises(InvalidRequest):
        drive(eng, dict(case, calls=1), (1,))
        eng.collect_events(2, 1)                                       # out of order
    with pytest.raises(InvalidRequest):
        eng.collect_events(0, 1)                                       # repeated
    with pytest.raises(InvalidRequest):
        eng.collect_events(1, -1)
    for c0, n in C.pieces_of((159,), case["calls"] - 1):
        eng.collect_events(1 + c0, n, case["handled"][1 + c0:1 + c0 + n], case["net"][1 + c0:1 + c0 + n])
    assert_matches(eng, C.run_model(case, spectator=True))
