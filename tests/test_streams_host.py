"""The stream rule of the device track table and the filler's arithmetic, without a device: stub streams that count synchronize() calls and
compare by identity stand in for torch's, and the filler gets its unit time injected."""
import numpy as np
import pytest
import torch

import stream_probe
from centernet_lightning_amd._track_host import TrackTable


class StubStream:
    def __init__(self):
        self.syncs = 0

    def synchronize(self):
        self.syncs += 1

    def __eq__(self, other):
        return self is other

    def __ne__(self, other):
        return self is not other

    __hash__ = object.__hash__


def _table(stream):
    t = TrackTable()
    t.stream = stream
    t.emb = torch.arange(12, dtype=torch.float32).reshape(3, 4)
    t.box = torch.arange(12, 24, dtype=torch.float32).reshape(3, 4)
    return t


def test_wait_synchronises_the_stored_stream_when_the_current_one_differs_or_is_none():
    a, b = StubStream(), StubStream()
    t = _table(a)
    t.wait_for_other_stream(a)
    assert (a.syncs, b.syncs) == (0, 0)                 # same stream: stream order does it
    t.wait_for_other_stream(b)
    assert (a.syncs, b.syncs) == (1, 0)                 # the STORED stream is finished, not the current one
    t.wait_for_other_stream(None)
    assert (a.syncs, b.syncs) == (2, 0)
    t.wait_for_other_stream()
    assert (a.syncs, b.syncs) == (3, 0)
    assert t.stream is a                                # waiting does not forget the stream


def test_wait_never_synchronises_before_the_first_update():
    a = StubStream()
    t = TrackTable()
    assert t.stream is None
    t.wait_for_other_stream(a)
    t.wait_for_other_stream(None)
    t.wait_for_other_stream()
    assert a.syncs == 0


def test_clear_always_waits_and_then_forgets_the_stream():
    a = StubStream()
    t = _table(a)
    t.clear()
    assert a.syncs == 1 and t.stream is None and t.emb is None and t.box is None
    t.clear()                                           # nothing to wait for any more
    assert a.syncs == 1
    t.wait_for_other_stream(StubStream())
    assert a.syncs == 1


def test_read_row_waits_under_the_same_condition_and_not_otherwise():
    a, b = StubStream(), StubStream()
    t = _table(a)
    row = t.read_row("emb", 1, a)
    assert (a.syncs, b.syncs) == (0, 0)
    assert isinstance(row, np.ndarray) and row.tobytes() == np.arange(4, 8, dtype=np.float32).tobytes()
    row = t.read_row("box", 2, b)
    assert (a.syncs, b.syncs) == (1, 0)
    assert row.tobytes() == np.arange(20, 24, dtype=np.float32).tobytes()
    t.read_row("emb", 0, b)
    assert (a.syncs, b.syncs) == (2, 0)                 # the read leaves `stream` as it was: the next read under b waits again
    t.stream = None                                     # a table no launch has written (rows set by hand)
    t.read_row("emb", 0, b)
    assert (a.syncs, b.syncs) == (2, 0)


def test_track_embedding_and_device_kalman_go_through_read_row(monkeypatch):
    from centernet_lightning_amd._track_host import DeviceKalman, Track
    seen = []

    class Settings:
        _table = TrackTable()

    monkeypatch.setattr(TrackTable, "read_row", lambda self, name, row, cur=None: seen.append((name, row)) or np.zeros(64))
    trk = Track(Settings, 0, np.zeros(4), 0, use_kalman="device")
    trk._row = 5
    assert isinstance(trk.kf, DeviceKalman)
    trk.embedding, trk.kf.x, trk.kf.P
    assert seen == [("emb", 5), ("kx", 5), ("kP", 5)]


@pytest.mark.parametrize("ms, unit, units", [(30.0, 0.5, 60), (30.1, 0.5, 61), (0.01, 0.5, 1), (1000.0, 0.3, 3334), (50.0, 50.0, 1), (50.0, 49.0, 2)])
def test_filler_rounds_up_to_whole_units(ms, unit, units):
    assert stream_probe.Filler(unit_ms=unit).units(ms) == units


@pytest.mark.parametrize("ms", [1000.001, 2000.0, float("inf"), 0.0, -1.0, float("nan")])
def test_filler_refuses_more_than_its_cap(ms):
    f = stream_probe.Filler(unit_ms=0.5)
    with pytest.raises(ValueError):
        f.units(ms)
    with pytest.raises(ValueError):
        f.queue(None, ms)                               # refused before anything touches a device
