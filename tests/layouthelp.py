"""Helpers of tests/test_gpu_layout.py: framed buffers (guard | payload | guard, all of it filled with a chosen pattern) in host or
device memory, placing bit streams into slots so that the spare bits of the last byte and everything behind it come from the fill,
and the comparisons with the oracle.  Nothing here touches the GPU unless a Frame is asked for device memory, so the comparisons
are tested without one (tests/test_layout_helpers.py)."""
import numpy as np

GUARD = 64 * 1024            # far beyond any read-ahead of the decoders (include/kanzi_hip.h: KZ_STREAM_SLACK = 64 bytes)
FILLS = ("zero", "ones", "rand")


def fill_bytes(fill, n, seed=0):
    if fill == "zero":
        return np.zeros(n, dtype=np.uint8)
    if fill == "ones":
        return np.full(n, 0xFF, dtype=np.uint8)
    if fill == "a5":
        return np.full(n, 0xA5, dtype=np.uint8)
    assert fill == "rand", fill
    return np.random.default_rng(0xF111 + seed).integers(0, 256, n, dtype=np.uint8)


class Frame:
    """guard | payload | guard.  `img` is the host image: write rows into it with put() / put_stream(), then ptr() hands out the
    address of payload byte `off` (device=True: the image is uploaded to one torch.uint8 tensor first).  after() is the whole frame
    as it is now; guards_intact() compares both guards with the fill, untouched() the whole frame with what was handed out."""

    def __init__(self, payload, fill, device=False, seed=0, guard=GUARD):
        self.payload, self.guard, self.device = int(payload), guard, device
        self.fill = fill_bytes(fill, guard + self.payload + guard, seed)
        self.img = self.fill.copy()
        self.t = None
        self.sent = None

    def put(self, off, data):
        a = np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) else data
        assert 0 <= off and off + len(a) <= self.payload, (off, len(a), self.payload)
        self.img[self.guard + off:self.guard + off + len(a)] = a

    def put_stream(self, off, stream, nbits):
        """the first nbits bits of `stream` at payload byte `off`; the spare bits of the last byte keep the fill"""
        nby = (nbits + 7) // 8
        assert len(stream) >= nby
        if nby == 0:
            return
        self.put(off, stream[:nby])
        spare = (-nbits) % 8
        if spare:
            m = (1 << spare) - 1
            i = self.guard + off + nby - 1
            self.img[i] = (stream[nby - 1] & ~m & 0xFF) | (int(self.fill[i]) & m)

    def ptr(self, off=0):
        if self.device:
            if self.t is None:
                import torch
                self.t = torch.from_numpy(self.img).cuda()
                self.sent = self.img.copy()
            return self.t.data_ptr() + self.guard + off
        if self.sent is None:
            self.sent = self.img.copy()
        return self.img.ctypes.data + self.guard + off

    def after(self):
        if self.device and self.t is not None:
            import torch
            torch.cuda.synchronize()
            return self.t.cpu().numpy()
        return self.img

    def rows(self, off, stride, n, width):
        a = self.after()
        return [a[self.guard + off + b * stride:self.guard + off + b * stride + width] for b in range(n)]

    def guards_intact(self, a=None):
        a = self.after() if a is None else a
        g, p = self.guard, self.payload
        return bool(np.array_equal(a[:g], self.fill[:g]) and np.array_equal(a[g + p:], self.fill[g + p:]))

    def untouched(self, a=None):
        a = self.after() if a is None else a
        return bool(np.array_equal(a, self.sent if self.sent is not None else self.fill))


def assert_guards(frame, tag, a=None):
    assert frame.guards_intact(a), ("guard bytes changed", tag)


def check_decoded(tag, status, length, got, ref_r, ref_bytes):
    """one block of kz_decode_blocks against oracle.decode_block of that stream alone: ref_r >= 0 is the decoded length (bytes
    compared), < 0 the error code.  -> True if the oracle accepted the stream"""
    if ref_r >= 0:
        assert status == 0 and length == ref_r, ("status / length", tag, status, length, ref_r)
        assert bytes(got[:ref_r]) == bytes(ref_bytes), ("decoded bytes", tag)
        return True
    assert status == ref_r, ("status", tag, status, ref_r)
    assert length == 0, ("length of a failed block", tag, length)
    return False


def check_entropy_decoded(tag, rc, got, used, count, ref_r, ref_bytes, ref_used):
    """kz_entropy_decode against the oracle's (or the ANS1 model's) decoder on exactly the same bits.  -> True if accepted"""
    if ref_r == count:
        assert rc == count, ("verdict", tag, rc)
        assert bytes(got[:count]) == bytes(ref_bytes[:count]), ("decoded bytes", tag)
        assert used == ref_used, ("bits consumed", tag, used, ref_used)
        return True
    assert rc < 0, ("verdict", tag, rc, ref_r)
    return False


def check_stream(tag, res, row, ref):
    """one block of kz_encode_blocks (res: its kz_block_result, row: its output row) against oracle.encode_block of the block
    alone: ref = (stream bytes, W, skipFlags, postLen)"""
    stream, w, sf, post = ref
    assert res.status == 0, ("status", tag, res.status)
    assert res.bits == w, ("bits", tag, res.bits, w)
    assert res.length == post, ("length", tag, res.length, post)
    nby = (w + 7) // 8
    assert bytes(row[:nby]) == bytes(stream[:nby]), ("stream bytes", tag)
    if w:
        assert res.skipFlags == sf, ("skipFlags", tag, res.skipFlags, sf)
        assert res.mode == stream[0], ("mode", tag, res.mode, stream[0])


def ragged_lengths():
    """around 16 / 33 / 16 384 / 32 768 / 40 000 / 65 536, with 0, 1, 15, 16, 32, 33 in the middle"""
    return [16385, 17, 32768, 0, 1, 40000, 15, 16, 65536, 32, 33, 34, 16383, 32769, 39999, 65535, 16384, 65521]


def oracle_map(fn, items, threads=8):
    """fn over items on a few threads (the oracle's C calls release the interpreter lock)"""
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(threads) as ex:
        return list(ex.map(fn, items, chunksize=max(1, len(items) // (threads * 8))))
