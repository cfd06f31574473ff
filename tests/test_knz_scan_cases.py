"""kz_knz_scan (host memory, no GPU) on the case set of tests/knzscan.py: against the Python model of the rule on every case and
every minChain; on intact streams against kz_knz_index; on damaged streams against what is stated for each (which blocks come back,
where the chains break, what knz_recover_index makes of it); its capacity and refusal rules; that bytes behind n change nothing;
and the coverage the set is meant to have, computed from the model.  Streams are built by the oracle."""
import ctypes

import numpy as np
import pytest

import kanzi_amd as kz
import knzrange
import knzscan as ks
import oracle


def _compress(chain, ent, bs, data, checksum):
    return oracle.compress(chain, ent, bs, data, jobs=2, checksum=checksum)


def _encode_block(chain, ent, bs, block, checksum):
    s, w, _, _ = oracle.encode_block(chain, ent, block, checksum=checksum, block_size=bs)
    return s, w


@pytest.fixture(scope="module")
def cases(built):
    return {c.name: c for c in ks.cases(_compress, _encode_block)}


@pytest.fixture(scope="module")
def accepted(cases):
    """name -> the model's accepted positions, computed once"""
    return {c.name: ks.accepted(c.knz) for c in cases.values() if c.kind != "header"}


def raw_scan(knz, min_chain, cap, n=None, tail=b"\0" * 16, nulls=()):
    """kz_knz_scan with poisoned arrays of cap + 4 entries -> (rc, the four arrays, head)"""
    L = kz.load_library()
    src = np.frombuffer(bytes(knz) + tail, dtype=np.uint8)
    cols = np.full((4, max(cap, 0) + 4), -77, dtype=np.int64)
    head = ctypes.c_int64(-77)
    hdr = [ctypes.c_uint64(0), ctypes.c_uint32(0), ctypes.c_int32(0), ctypes.c_int64(0), ctypes.c_int32(0)]
    args = [src.ctypes.data, len(knz) if n is None else n, min_chain] + [ctypes.addressof(h) for h in hdr] + \
           [cols[k].ctypes.data for k in range(4)] + [cap, ctypes.addressof(head)]
    for k in nulls:
        args[k] = None
    return L.kz_knz_scan(*args), cols, head.value


def same(scan, want):
    return all(scan[k] == want[k] for k in ("prefix", "blocks", "next", "head"))


def test_the_binding_declares_the_calls(built):
    L = ctypes.CDLL(kz.LIB_PATH)
    for name in ("kz_knz_scan", "kz_knz_scan_device"):
        assert name in kz.ABI_SYMBOLS and hasattr(L, name), name
    for name in ("knz_scan", "knz_scan_device", "knz_recover_index", "knz_salvage"):
        assert hasattr(kz, name), name
    assert (kz.SCAN_END, kz.SCAN_BROKEN) == (ks.END, ks.BROKEN) == (-1, -2)
    assert kz.load_library().kz_abi_version() == 3


def test_the_scan_is_the_model(cases, accepted):
    for name, acc in accepted.items():
        for mc in ks.MIN_CHAINS:
            got, want = kz.knz_scan(cases[name].knz, mc), ks.model(cases[name].knz, mc, acc)
            assert same(got, want), (name, mc, len(got["prefix"]), len(want["prefix"]), got["head"], want["head"])


def test_intact_streams_give_the_index(cases):
    for c in cases.values():
        if c.kind != "intact":
            continue
        idx, scan = kz.knz_index(c.knz), kz.knz_scan(c.knz, 4)
        for k in ("transform", "entropy", "blockSize", "inputSize", "checksum"):
            assert scan[k] == idx[k], (c.name, k)
        path, end = ks.chain(scan, scan["head"])
        assert end == ks.END and [scan["blocks"][i] for i in path] == idx["blocks"], c.name
        assert len(scan["blocks"]) == len(idx["blocks"]), (c.name, "entries off the stream's chain")
        assert scan["prefix"] == [p for p, _, _ in knzrange.fields(c.knz, idx)], c.name
        assert scan["headerBits"] == knzrange.header_bits(c.knz) and scan["streamBits"] == 8 * len(c.knz)
        assert kz.knz_recover_index(scan) == (list(range(len(idx["blocks"]))), []), c.name


def test_incompressible_payload(cases, accepted):
    c = cases["random-256k"]
    true = set(kz.knz_index(c.knz)["blocks"])
    off = {mc: [b for b in ks.model(c.knz, mc, accepted[c.name])["blocks"] if b not in true] for mc in (1, 2, 4)}
    assert len(off[1]) >= 50 and len(off[4]) == 0 and len(off[2]) <= len(off[1]), {mc: len(v) for mc, v in off.items()}
    for mc in (1, 2, 4):
        scan = kz.knz_scan(c.knz, mc)
        assert true <= set(scan["blocks"]) and len(scan["blocks"]) == len(true) + len(off[mc]), mc
        assert [scan["blocks"][i] for i in ks.chain(scan, scan["head"])[0]] == kz.knz_index(c.knz)["blocks"], mc


def test_a_nested_stream_is_a_chain_of_its_own(cases):
    c = cases["nested"]
    scan = kz.knz_scan(c.knz, 4)
    own, end = ks.chain(scan, scan["head"])
    assert end == ks.END and [scan["blocks"][i] for i in own] == kz.knz_index(c.knz)["blocks"] and len(own) == 1
    inner = [i for i in range(len(scan["prefix"])) if i not in own]
    assert len(inner) == c.info["inner_blocks"]
    path, end = ks.chain(scan, inner[0])
    assert path == inner and end == ks.BROKEN                      # the inner end marker is not the stream's last byte
    o, w = scan["blocks"][own[0]]
    assert all(o < scan["prefix"][i] and sum(scan["blocks"][i]) <= o + w for i in inner)
    assert kz.knz_recover_index(scan) == (own, [])                 # only head says which chain is the stream's


def test_entries_inside_the_block_in_front_of_a_break(cases):
    """knz_recover_index counts the last block of a chain that ends BROKEN as taken up to its payload's first bit only, so kept
    entries inside it are taken with their chains: the nested stream's, once the stream is cut behind the block that holds it"""
    c = cases["nested"]
    cut = c.knz[:-1]                                               # the end marker gone: the block is whole, its chain ends BROKEN
    scan = kz.knz_scan(cut, 1)                                     # (a lone block that does not reach the end marker: kept at minChain 1 only)
    assert scan["head"] == 0 and scan["next"][0] == ks.BROKEN and scan["blocks"][0] == kz.knz_index(c.knz)["blocks"][0]
    whole = kz.knz_scan(c.knz, 4)
    inner = [b for b in whole["blocks"] if b != whole["blocks"][whole["head"]]]
    entries, gaps = kz.knz_recover_index(scan)
    taken = [scan["blocks"][i] for i in entries]
    assert taken[0] == scan["blocks"][0] and [b for b in taken if b in inner] == inner and gaps == [], (entries, gaps)
    assert kz.knz_scan(cut, 4)["head"] == ks.BROKEN and [b for b in kz.knz_scan(cut, 4)["blocks"]] == inner
    assert kz.knz_recover_index(kz.knz_scan(c.knz, 1))[0] == [0]   # the same entries inside a block of an unbroken chain: passed over


def test_damaged_streams(cases):
    for c in cases.values():
        if c.kind != "damage":
            continue
        info = c.info
        for mc, lost, broken, gaps in ((4, info["lost"], info["broken_after"], info["gaps"]),
                                       (3, set(info.get("lost3", info["lost"])), info.get("broken_after3", info["broken_after"]), info.get("gaps3", info["gaps"]))):
            scan = kz.knz_scan(c.knz, mc)
            want = [b for k, b in enumerate(info["where"]) if k not in lost]
            assert scan["blocks"] == want, (c.name, mc)
            place = {b: i for i, b in enumerate(scan["blocks"])}
            for k, b in enumerate(info["where"]):
                if k in lost:
                    continue
                nxt = scan["next"][place[b]]
                if k in broken:
                    assert nxt == ks.BROKEN, (c.name, mc, k)
                elif k == 11:
                    assert nxt == ks.END, (c.name, mc, k)
                else:
                    assert nxt == place[info["where"][k + 1]], (c.name, mc, k)
            assert scan["head"] == 0, (c.name, mc)
            entries, got_gaps = kz.knz_recover_index(scan)
            assert entries == list(range(len(want))) and got_gaps == gaps, (c.name, mc, entries, got_gaps, gaps)
        if info.get("same_as_base"):
            assert same(kz.knz_scan(c.knz, 4), kz.knz_scan(info["base"], 4)), c.name


def test_a_damaged_stream_header_gives_its_code(cases):
    c = cases["flip-stream-header"]
    L = kz.load_library()
    src = np.frombuffer(c.knz + b"\0" * 16, dtype=np.uint8)
    code = L.kz_knz_index(src.ctypes.data, len(c.knz), None, None, None, None, None, None, None, 0)
    rc, cols, head = raw_scan(c.knz, 4, 8)
    assert rc == code and code < 0 and head == -77 and bool((cols == -77).all()), (rc, code)
    with pytest.raises(kz.KanziError) as e:
        kz.knz_scan(c.knz)
    assert e.value.code == -code


def test_capacity(cases):
    for name in ("bwt-1k-5-short-last", "damage-base"):
        knz = cases[name].knz
        full = kz.knz_scan(knz, 4)
        k = len(full["prefix"])
        for cap in (k, k - 1, 0):
            rc, cols, head = raw_scan(knz, 4, cap)
            assert rc == k and head == full["head"], (name, cap, rc)
            for col, key in ((0, "prefix"), (3, "next")):
                assert cols[col][:cap].tolist() == full[key][:cap], (name, cap, key)       # next points by index, below cap or not
            assert [tuple(x) for x in zip(cols[1][:cap].tolist(), cols[2][:cap].tolist())] == full["blocks"][:cap], (name, cap)
            assert bool((cols[:, cap:] == -77).all()), (name, cap, "entries behind cap")
    rc, _, head = raw_scan(cases["one"].knz, 4, 0, nulls=(8, 9, 10, 11))                       # cap == 0: the arrays may be null
    assert rc == 1 and head == 0


def test_refusals(cases):
    knz = cases["none-1k-3"].knz
    for what, kw in (("n < 0", dict(n=-1)), ("cap < 0", dict(cap=-1)), ("minChain 0", dict(min_chain=0)), ("minChain < 0", dict(min_chain=-3)),
                     ("src", dict(nulls=(0,))), ("head", dict(nulls=(13,))), ("prefixBitOff", dict(nulls=(8,))), ("blockBitOff", dict(nulls=(9,))),
                     ("blockBits", dict(nulls=(10,))), ("next", dict(nulls=(11,)))):
        a = dict(min_chain=4, cap=8)
        a.update(kw)
        rc, cols, head = raw_scan(knz, a["min_chain"], a["cap"], n=a.get("n"), nulls=a.get("nulls", ()))
        assert rc == -18 and bool((cols == -77).all()) and head == -77, (what, rc)
    L = kz.load_library()
    for n in (0, 19):                                               # kz_knz_index's code for a stream too short for a header
        assert raw_scan(knz, 4, 8, n=n)[0] == L.kz_knz_index(np.frombuffer(knz, dtype=np.uint8).ctypes.data, n, None, None, None, None, None, None, None, 0) == -15
    rc, _, head = raw_scan(knz, 4, 8, nulls=(3, 4, 5, 6, 7))       # the header out-pointers may be null
    assert rc == 3 and head == 0


def test_bytes_behind_n_change_nothing(cases, accepted):
    rng = np.random.default_rng(4)
    for name in ("seams", "cut", "lz-fpaq-4k-x64-copy-last", "empty"):
        knz = cases[name].knz
        want = raw_scan(knz, 1, 4096, tail=b"\0" * 16)
        for tail in (b"\xff" * 16, rng.integers(0, 256, 16, dtype=np.uint8).tobytes(), knz[-16:]):
            got = raw_scan(knz, 1, 4096, tail=tail)
            assert got[0] == want[0] and got[2] == want[2] and bool((got[1] == want[1]).all()), name
    # the same bytes as the front of a longer buffer: n decides, not the buffer
    knz = cases["cut"].knz
    whole = cases["damage-base"].knz
    assert whole[:len(knz)] == knz
    a, b = raw_scan(whole, 4, 64, n=len(knz), tail=b""), raw_scan(knz, 4, 64)
    assert a[0] == b[0] and a[2] == b[2] and bool((a[1] == b[1]).all())


def test_coverage(cases, accepted):
    """what the case set is meant to exercise, from the model's accepted positions on the streams' own chains"""
    lrs, forms, phases, seams, last16, copies = set(), set(), set(), set(), False, 0
    for c in cases.values():
        if c.kind != "intact":
            continue
        scan = ks.model(c.knz, 4, accepted[c.name])
        got = kz.knz_scan(c.knz, 4)
        assert got["prefix"] == scan["prefix"] and got["blocks"] == scan["blocks"], c.name      # what is counted below is what the library returns
        assert got["headerBits"] == ks.header(c.knz)[0] == 160 + 16 * kz._size_field_units(got["inputSize"]), c.name
        for q, (pay, w) in zip(scan["prefix"], scan["blocks"]):
            lrs.add(pay - q - 5)
            mode = ks._bits(c.knz, pay, 8)
            nbf = ks.header(c.knz)[1]
            forms.add(bool(mode & 0x10) and (not (mode & 0x80) or nbf > 4))
            copies += 1 if mode & 0x80 else 0
            phases.add(q % 8)
            for s in ks.SEAMS:
                by = q >> 3
                if by >= s - 16 and (by % s >= s - 16):
                    seams.add((s, "front"))
                if by >= s and (by % s < 16):
                    seams.add((s, "behind"))
            last16 = last16 or (q >> 3) >= len(c.knz) - 16
    # every width of the length field that the writer emits for blocks of 4 bytes (W = 56: 6 bits) to 64 KiB (W >= 2^19: 20 bits)
    assert set(range(6, 21)) <= lrs, sorted(lrs)
    assert forms == {False, True} and copies >= 3 and phases == set(range(8)), (forms, copies, phases)
    assert seams == {(s, side) for s in ks.SEAMS for side in ("front", "behind")} and last16, sorted(seams)
