"""CPU: the ctypes binding's finalizers in the wrong order.  alch_buf_free, alch_hint_free and alch_tunnel_free reach into the ring
their handle belongs to (its buffer pool, its device lock), and Python runs the finalizers of a garbage cycle -- the frames of a
failed test, for one -- in any order.  A handle whose ring has been destroyed already is dropped, never passed to the library: on a
GPU the call wrote into freed host memory and aborted the process at some later allocation.  A recording stand-in for the library
shows which calls the binding makes."""
from alchemy_amd import capi


class RecordingLib:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        return lambda *args: self.calls.append(name) or 0


def make():
    lib = RecordingLib()
    rings = []
    for _ in range(2):
        r = capi.Ring.__new__(capi.Ring)
        r._l, r._h = lib, object()
        rings.append(r)
    buf = capi.Buf.__new__(capi.Buf)
    buf.ring, buf.n_elems, buf._h = rings[0], 1, object()
    hint = capi.Hint(rings[0], object())
    tun = capi.Tunnel.__new__(capi.Tunnel)
    tun.ring_r, tun.ring_s, tun._h = rings[0], rings[1], object()
    return lib, rings, buf, hint, tun


def test_children_freed_before_their_ring_reach_the_library():
    lib, rings, buf, hint, tun = make()
    for x in (tun, hint, buf):
        x.free()
        x.free()                                                   # a second free is a no-op
    for r in rings:
        r.close()
    assert lib.calls == ["alch_tunnel_free", "alch_hint_free", "alch_buf_free", "alch_ring_destroy", "alch_ring_destroy"]


def test_children_freed_after_their_ring_do_not():
    lib, rings, buf, hint, tun = make()
    rings[0].close()                                               # the ring of buf and hint, and the tunnel's source ring
    for x in (buf, hint, tun):
        x.free()
        assert x._h is None
    rings[1].close()
    assert lib.calls == ["alch_ring_destroy", "alch_ring_destroy"]
