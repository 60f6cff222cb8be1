"""Load for the stream-ordering tests (tests/test_gpu_stream_order.py): work that keeps a chosen stream busy while the call under
test is issued, so that queue order no longer equals issue order and a missing wait shows as wrong words.

Ballast(stream_of)   a two-power ring of its own, made to queue on the stream under test: `stream_of` is a Ring (its stream is
                     borrowed with share_stream, whoever owns it) or a hipStream_t as an int (a caller-owned stream, 0 = the null
                     stream: set_stream).  push(k) queues k in-place crt; crtinv round trips on one resident buffer, without any
                     synchronisation.  A round trip is a bit-exact identity, so the buffer never changes and one Ballast serves any
                     number of pushes; nothing ever reads its results.
busy(stream)         non-blocking: True while the stream still has queued work.  `stream` is a torch.cuda.Stream, a Ring (the stream
                     alch_ring_device reports) or a hipStream_t as an int.

Every loaded case asserts busy(loaded stream) right after the call under test has returned and before any download or
synchronisation: if the ballast had already drained, the case proved nothing and fails.

Sizing (MI355X, measured once):
  (a) host time of the slowest call under test to return on idle streams, time.perf_counter around the call, five calls after a
      warm-up: 0.29 ms at most (median 0.26 ms) for the eight-chunk alch_ct_tunnel 11648 -> 29120 with tunnel_ep = 0; the other
      tunnels 0.03 .. 0.12 ms, the unfused alch_ct_mul_full 0.17 ms, two alch_ct_mul_relin calls back to back 0.06 .. 0.11 ms,
      modSwitch / embed / twace / coeffs 0.015 .. 0.04 ms.
  (b) one ballast round trip (crt; crtinv of ELEMS = 96 elements of the ring below), Ring.timer_start / timer_stop over 32 round
      trips divided by 32: 0.103 ms (0.057 ms at 32 elements, 0.21 ms at 256).  Queuing one costs the host 0.007 ms, so the queue
      grows fifteen times faster than it drains.
  The queued ballast must last at least 50 (a) -- the margin covers host jitter on a shared machine -- and at most 100 ms:
  K_DEFAULT = ceil(50 (a) / (b)) = 141 round trips = 14.5 ms, checked below from the two constants.
"""
import math

import alchemy_amd as A

# the ballast ring: m = 2^16 (n = 2^15, the largest LDS-resident transform), four limbs, 32-bit words
BALLAST_M = 1 << 16
BALLAST_QS = [2147352577, 2146959361, 2146041857, 2145976321]
ELEMS = 96                                       # 96 elements x 4 limbs x 2^15 words x 4 B = 48 MiB per pass, read and written

A_SLOWEST_CALL_MS = 0.29                         # (a), measured
B_ROUND_TRIP_MS = 0.103                          # (b), measured
MARGIN = 50
K_DEFAULT = math.ceil(MARGIN * A_SLOWEST_CALL_MS / B_ROUND_TRIP_MS)
assert K_DEFAULT * B_ROUND_TRIP_MS >= MARGIN * A_SLOWEST_CALL_MS
assert K_DEFAULT * B_ROUND_TRIP_MS <= 100.0, "the ballast of one case must not last longer than 100 ms"


def stream_ptr(stream) -> int:
    """hipStream_t as an int of a torch stream, a Ring or an int."""
    if isinstance(stream, int):
        return stream
    if isinstance(stream, A.Ring):
        return stream.device_stream()[1]
    return int(stream.cuda_stream)


def busy(stream) -> bool:
    import torch
    if isinstance(stream, torch.cuda.Stream):
        return not stream.query()
    ptr = stream_ptr(stream)
    if ptr == 0:
        s = torch.cuda.default_stream()
        assert s.cuda_stream == 0                # torch's default stream is HIP's null stream
        return not s.query()
    return not torch.cuda.ExternalStream(ptr).query()


class Ballast:
    def __init__(self, stream_of, elems: int = ELEMS):
        self.ring = A.Ring(BALLAST_M, BALLAST_QS)
        self.buf = self.ring.alloc(elems)
        self.buf.fill_uniform(0xBA11A57)
        self.bind(stream_of)

    def bind(self, stream_of):
        """Queue on another stream from now on (both calls first wait for what the ballast ring has queued so far)."""
        if isinstance(stream_of, A.Ring):
            self.ring.share_stream(stream_of)
        else:
            self.ring.set_stream(stream_ptr(stream_of))

    def push(self, k: int = K_DEFAULT):
        for _ in range(k):
            self.buf.crt()
            self.buf.crtinv()

    def round_trip_ms(self, k: int = 32) -> float:
        """(b): mean time of one round trip on an otherwise idle stream."""
        self.push(2)
        self.ring.sync()
        self.ring.timer_start()
        self.push(k)
        return self.ring.timer_stop() / k

    def close(self):
        self.buf.free()
        self.ring.close()
