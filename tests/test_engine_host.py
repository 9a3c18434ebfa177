"""The engine cache's contract (lav_amd.engine.Engine), on a tiny module with a counting builder: no library, no GPU."""
import torch
from torch import nn

from lav_amd.engine import Engine

CPU, META = torch.device("cpu"), torch.device("meta")     # (two device values: the cache only compares them)


class Packed:
    def __init__(self):
        self.refreshed = 0

    def refresh(self):
        self.refreshed += 1


class Tiny(Engine):
    def __init__(self):
        super().__init__()
        self.lin = nn.Linear(3, 2)
        self.bn = nn.BatchNorm1d(2)
        self.built = 0

    def build(self):
        self.built += 1
        return dict(layers=[Packed()])

    def engine(self, device=CPU, key="k"):
        return self._engine_for(device, key, self.build)


class TinyCopy(Tiny):
    """An engine of plain copies: nothing to refresh, so in-place changes drop it."""

    def _mark_stale(self):
        self._drop()


def _refreshed(e):
    return e["layers"][0].refreshed


def test_same_key_is_cached_and_other_keys_sit_beside_it():
    m = Tiny().eval()
    e = m.engine()
    assert m.engine() is e and m.built == 1
    other = m.engine(key=("k", 1))
    assert other is not e and m.built == 2
    assert m.engine() is e and m.engine(key=("k", 1)) is other and m.built == 2
    assert set(m._eng) == {"device", "tensor_ids", "k", ("k", 1)} and m._eng["device"] == CPU
    assert m._eng["tensor_ids"] == m._tensor_ids()


def test_another_device_rebuilds():
    m = Tiny().eval()
    e = m.engine(CPU)
    e2 = m.engine(META)
    assert e2 is not e and m.built == 2 and m._eng["device"] == META and "k" in m._eng
    assert m.engine(META) is e2 and m.built == 2


def test_mode_toggle_refreshes_once_at_the_next_use():
    m = Tiny().eval()
    e = m.engine()
    m.train(); m.eval()
    assert _refreshed(e) == 0                      # nothing happens until the engine is used
    assert m.engine() is e and _refreshed(e) == 1 and m.built == 1
    assert m.engine() is e and _refreshed(e) == 1  # and none after that
    m.eval(); m.eval()                             # the mode did not change: nothing is stale
    assert m.engine() is e and _refreshed(e) == 1
    m.train(); m.train()
    m.eval()
    assert m.engine() is e and _refreshed(e) == 2


def test_every_key_of_a_stale_engine_is_refreshed():
    m = Tiny().eval()
    a, b = m.engine(key="a"), m.engine(key="b")
    m.train(); m.eval()
    assert m.engine(key="a") is a and (_refreshed(a), _refreshed(b)) == (1, 1)


def test_load_state_dict_refreshes_once():
    m = Tiny().eval()
    e = m.engine()
    m.load_state_dict({k: v + 1 for k, v in m.state_dict().items()})
    assert m.engine() is e and _refreshed(e) == 1 and m.built == 1
    assert m.engine() is e and _refreshed(e) == 1


def test_load_state_dict_assign_rebuilds():
    m = Tiny().eval()
    e = m.engine()
    m.load_state_dict({k: v.clone() for k, v in m.state_dict().items()}, assign=True)    # parameter objects are replaced
    e2 = m.engine()
    assert e2 is not e and m.built == 2 and _refreshed(e) == 0 and _refreshed(e2) == 0
    assert m._eng["tensor_ids"] == m._tensor_ids()
    m.lin.weight = nn.Parameter(torch.zeros(2, 3))       # so does an assignment; noticed at the next event that marks stale
    m.train(); m.eval()
    assert m.engine() is not e2 and m.built == 3


def test_apply_drops_the_engine():
    m = Tiny().eval()
    e = m.engine()
    m.float()
    assert m._eng is None
    assert m.engine() is not e and m.built == 2 and _refreshed(e) == 0


def test_engine_of_copies_rebuilds_on_a_toggle_only():
    m = TinyCopy().eval()
    e = m.engine()
    m.eval(); m.eval()
    assert m.engine() is e and m.built == 1              # a same-mode call does not rebuild
    m.train(); m.eval()
    e2 = m.engine()
    assert e2 is not e and m.built == 2 and _refreshed(e) == 0
    m.load_state_dict(m.state_dict())
    assert m.engine() is not e2 and m.built == 3
    m.float()
    assert m._eng is None


def test_a_child_engine_follows_its_parent():
    """train() / load_state_dict / _apply reach an Engine that sits inside a plain nn.Module."""
    outer = nn.Sequential(Tiny(), TinyCopy()).eval()
    a, b = outer[0].engine(), outer[1].engine()
    outer.train(); outer.eval()
    assert outer[0].engine() is a and _refreshed(a) == 1
    assert outer[1].engine() is not b
    outer.load_state_dict(outer.state_dict())
    assert outer[0].engine() is a and _refreshed(a) == 2
    outer.double()
    assert outer[0]._eng is None and outer[1]._eng is None
