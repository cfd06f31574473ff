"""kz_knz_scan_device against kz_knz_scan on the case set of tests/knzscan.py, array for array and return value for return value:
the host form is the reference throughout (tests/test_knz_scan_cases.py holds it to the Python model).  The stream lies at odd
base addresses inside a poisoned device buffer, with different poison behind it from run to run; then the salvage of damaged
streams end to end, and the scan against the serial walk on a stream of 20 000 blocks."""
import ctypes

import numpy as np
import pytest

import kanzi_amd as kz
import datagen
import knzscan as ks
import oracle

pytestmark = pytest.mark.gpu

BASES = (0, 1, 7, 15)
POISONS = (0xA5, 0x00)             # behind n: a byte pattern, and zeros (which read as end markers)
LEAD = 64                          # poisoned bytes in front of the stream, 16-byte aligned with the buffer


def _compress(chain, ent, bs, data, checksum):
    return oracle.compress(chain, ent, bs, data, jobs=2, checksum=checksum)


def _encode_block(chain, ent, bs, block, checksum):
    s, w, _, _ = oracle.encode_block(chain, ent, block, checksum=checksum, block_size=bs)
    return s, w


@pytest.fixture(scope="module")
def cases(built):
    return {c.name: c for c in ks.cases(_compress, _encode_block)}


def _call(fn, front, src, n, min_chain, cap, nulls=()):
    """a scan call with poisoned arrays of cap + 4 entries -> (rc, header fields, the four arrays, head)"""
    cols = np.full((4, max(cap, 0) + 4), -77, dtype=np.int64)
    head = ctypes.c_int64(-77)
    hdr = [ctypes.c_uint64(0), ctypes.c_uint32(0), ctypes.c_int32(0), ctypes.c_int64(0), ctypes.c_int32(0)]
    args = list(front) + [src, n, min_chain] + [ctypes.addressof(h) for h in hdr] + [cols[k].ctypes.data for k in range(4)] + [cap, ctypes.addressof(head)]
    for k in nulls:
        args[len(front) + k] = None
    return fn(*args), [h.value for h in hdr], cols, head.value


def host(knz, min_chain, cap, **kw):
    src = np.frombuffer(bytes(knz) + b"\0" * 16, dtype=np.uint8)
    return _call(kz.load_library().kz_knz_scan, (), src.ctypes.data, len(knz), min_chain, cap, **kw)


def on_device(knz, base, poison):
    """the stream `base` bytes behind a 16-byte boundary of a poisoned device buffer -> (tensor, the stream's address)"""
    import torch
    buf = np.full(LEAD + base + len(knz) + 64, poison, dtype=np.uint8)
    buf[LEAD + base:LEAD + base + len(knz)] = np.frombuffer(knz, dtype=np.uint8)
    t = torch.from_numpy(buf).cuda()
    torch.cuda.synchronize()
    assert t.data_ptr() % 16 == 0
    return t, t.data_ptr() + LEAD + base


def device(ctx, addr, n, min_chain, cap, **kw):
    return _call(ctx.lib.kz_knz_scan_device, (ctx.h,), addr, n, min_chain, cap, **kw)


def equal(a, b):
    return a[0] == b[0] and a[1] == b[1] and a[3] == b[3] and bool((a[2] == b[2]).all())


def _device_equals_host(ctx, c):
    want = {mc: host(c.knz, mc, max(host(c.knz, mc, 0)[0], 0)) for mc in ks.MIN_CHAINS}
    for base in BASES:
        for poison in POISONS:
            t, addr = on_device(c.knz, base, poison)
            for mc in ks.MIN_CHAINS:
                got = device(ctx, addr, len(c.knz), mc, max(want[mc][0], 0))
                assert equal(got, want[mc]), (c.name, base, poison, mc, got[0], want[mc][0], got[3], want[mc][3])
            del t


def test_device_equals_host(ctx, cases):
    for c in cases.values():
        if c.name != "many-64":
            _device_equals_host(ctx, c)


def test_device_equals_host_on_many_tiles(ctx, cases):
    _device_equals_host(ctx, cases["many-64"])


def test_a_fresh_context_grows_its_tables_between_the_passes(built, cases):
    """The first large call of a context: the table buffer holds the tiles' first indices when it has to grow for the accepted
    positions (20 000 here, more than the first megabyte holds), and the count pass must run again whatever address the new
    allocation gets.  Contexts come and go, so that a freed table's address is there to be handed out again."""
    c = cases["many-64"]
    want = host(c.knz, 4, 20000)
    assert want[0] == 20000
    t, addr = on_device(c.knz, 1, 0xA5)
    for _ in range(3):
        fresh = kz.Context(0)
        try:
            assert equal(device(fresh, addr, len(c.knz), 4, 20000), want)
            assert equal(device(fresh, addr, len(c.knz), 4, 20000), want)        # and with the tables as they are now
        finally:
            fresh.close()


def test_capacity_and_refusals(ctx, cases):
    knz = cases["damage-base"].knz
    t, addr = on_device(knz, 3, 0xA5)
    k = host(knz, 4, 0)[0]
    assert k == 12
    for cap in (k, k - 1, 0):
        got, want = device(ctx, addr, len(knz), 4, cap), host(knz, 4, cap)
        assert got[0] == k and equal(got, want) and bool((got[2][:, cap:] == -77).all()), cap
    assert device(ctx, addr, len(knz), 4, 0, nulls=(8, 9, 10, 11))[0] == k
    for what, a in (("n < 0", dict(n=-1)), ("cap < 0", dict(cap=-1)), ("minChain", dict(mc=0)), ("src", dict(nulls=(0,))), ("head", dict(nulls=(13,))),
                    ("next", dict(nulls=(11,)))):
        got = device(ctx, addr, a.get("n", len(knz)), a.get("mc", 4), a.get("cap", 8), nulls=a.get("nulls", ()))
        assert got[0] == -18 and got[3] == -77 and bool((got[2] == -77).all()), (what, got[0])
    assert _call(ctx.lib.kz_knz_scan_device, (None,), addr, len(knz), 4, 8)[0] == -18
    assert device(ctx, addr, 19, 4, 8)[0] == -15                                 # too short for a stream header: kz_knz_index's code
    # a damaged stream header: the host form's code, and the text the other device calls give
    bad = cases["flip-stream-header"].knz
    t2, addr2 = on_device(bad, 5, 0xA5)
    got, want = device(ctx, addr2, len(bad), 4, 8), host(bad, 4, 8)
    assert got[0] == want[0] < 0 and got[3] == -77 and bool((got[2] == -77).all())
    assert ctx.lib.kz_knz_index_device(ctx.h, addr2, len(bad), None, None, None, None, None, None, None, 0) == got[0]
    v = bytearray(knz)
    v[4] = (v[4] & 0x0F) | 0x60                                                  # bitstream version 6
    t3, addr3 = on_device(bytes(v), 0, 0xA5)
    assert device(ctx, addr3, len(v), 4, 8)[0] == -16 and "version" in ctx.error()


def _blocks_of(base_data, bs):
    return [base_data[i:i + bs].tobytes() for i in range(0, len(base_data), bs)]


def test_salvage_end_to_end(ctx, cases):
    import torch
    original = _blocks_of(datagen.stream(12, 1024), 1024)
    for name, mc, absent in (("byte-deleted", 4, set()), ("two-breaks", 3, {5, 9}), ("two-breaks", 4, {5, 6, 7, 8, 9})):
        c = cases[name]
        t = torch.from_numpy(np.frombuffer(c.knz, dtype=np.uint8).copy()).cuda()
        got = kz.knz_salvage(ctx, t, mc)
        assert got == kz.knz_salvage(ctx, c.knz, mc), (name, mc, "device tensor and bytes")
        where = {b: k for k, b in enumerate(c.info["where"])}
        seen = {}
        for prefix, off, bits, status, data in got:
            k = where[(off, bits)]
            seen[k] = status
            if k in c.info.get("bad_decode", ()):
                assert status < 0 and data is None, (name, k, status)
            else:
                assert status == 0 and data == original[k], (name, k, status)
        assert sorted(seen) == [k for k in range(12) if k not in absent], (name, mc, sorted(seen))


def test_against_the_walk(ctx, cases):
    knz = cases["many-64"].knz
    t, addr = on_device(knz, 7, 0xA5)
    idx = kz.knz_index_device(ctx, addr, len(knz))
    scan = kz.knz_scan_device(ctx, addr, len(knz))
    path, end = ks.chain(scan, scan["head"])
    assert end == ks.END and len(path) == 20000 and [scan["blocks"][i] for i in path] == idx["blocks"]
    for k in ("transform", "entropy", "blockSize", "inputSize", "checksum"):
        assert scan[k] == idx[k], k
    assert scan["headerBits"] == ks.header(knz)[0] and scan["streamBits"] == 8 * len(knz)
