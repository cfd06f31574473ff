"""The batched block ABI under the layouts real callers use, and with stale memory everywhere the calls may look (the contract is
written at kz_encode_blocks / kz_decode_blocks in include/kanzi_hip.h): streams and blocks sit in framed buffers (64 KiB guards,
everything filled with 0x00, 0xFF or random bytes) at odd base offsets and strides, the spare bits of a stream's last byte and all
that follows it come from the fill, the context's arena holds another batch's data, and batches are larger than one launch.

The reference for every comparison is the CPU oracle run on ONE block alone with exactly its bytes / bits (for ANS1, which the C
oracle does not have, tests/ans1model.py and _ans1_block_from_none of tests/test_gpu_ans1.py).  No layout outside the contract is
ever handed to a kernel: those are exercised through the early -KZ_ERR_INVALID_PARAM only.  The comparisons themselves are shown
to bite, without a GPU, in tests/test_layout_helpers.py."""
import ctypes

import numpy as np
import pytest

import ans1model
import datagen
import katmodels
import kanzi_amd as kz
import oracle
import refinputs
import textgen
import layouthelp as lh
from layouthelp import FILLS, Frame

pytestmark = pytest.mark.gpu

BS = 65536
SLACK = 64                                     # KZ_STREAM_SLACK of include/kanzi_hip.h
CHAINS = ["BWT+RANK+ZRLT", "LZ", "BWT+SRT+ZRLT", "PACK+MM+LZX", "ZRLT", "NONE", "TEXT+UTF+BWT+RANK+ZRLT"]
# a pairwise-covering subset of chains x coders: every chain twice, ANS0 / FPAQ four times, HUFFMAN / NONE three times
COMBOS = [("BWT+RANK+ZRLT", "ANS0"), ("BWT+RANK+ZRLT", "HUFFMAN"), ("LZ", "HUFFMAN"), ("LZ", "ANS0"),
          ("BWT+SRT+ZRLT", "FPAQ"), ("BWT+SRT+ZRLT", "NONE"), ("PACK+MM+LZX", "HUFFMAN"), ("PACK+MM+LZX", "FPAQ"),
          ("ZRLT", "NONE"), ("ZRLT", "FPAQ"), ("NONE", "ANS0"), ("NONE", "NONE"),
          ("TEXT+UTF+BWT+RANK+ZRLT", "ANS0"), ("TEXT+UTF+BWT+RANK+ZRLT", "FPAQ")]
ANS1_CHAINS = ["NONE", "BWT+RANK+ZRLT", "LZ"]


def _ans1_block_from_none(*a):
    from test_gpu_ans1 import _ans1_block_from_none as f
    return f(*a)


def _blocks(lengths=None, first=0):
    """datagen classes 0-4 at the ragged lengths"""
    lengths = lh.ragged_lengths() if lengths is None else lengths
    return [datagen.block(first + i, max(n, 1))[:n].tobytes() for i, n in enumerate(lengths)]


def _encode_ref(chain, ent, data):
    """(stream, W, skipFlags, postLen) of one block alone; ANS1 from the block the oracle writes under NONE"""
    if ent != "ANS1":
        return oracle.encode_block(chain, ent, data, block_size=BS)
    s, w, sf, pl = oracle.encode_block(chain, "NONE", data, block_size=BS)
    if w == 0:
        return s, w, sf, pl
    s1, w1 = _ans1_block_from_none(s, w, len(data), len(chain.split("+")))
    return s1, w1, sf, pl


def _decode_ref(chain, ent, stream, nbits):
    return oracle.decode_block(chain, ent, BS, stream[:(nbits + 7) // 8], nbits, BS)


def _keep_len(bad, n):
    return (bytes(bad) + bytes(n))[:n]


def _damaged(rng, stream, i):
    """stream i of a batch damaged in place, its length kept: refinputs.corrupt kinds 0, 2, 4, 6, 7 in turn, and in between the
    mild kinds the oracle often still accepts (a single flip in the last 2 %, a zeroed tail of a few bytes)"""
    n = len(stream)
    k = i % 8
    if k < 5:
        return _keep_len(refinputs.corrupt(rng, stream, (0, 2, 4, 6, 7)[k]), n)
    bad = bytearray(stream)
    if k == 5 or n < 8:
        pos = n - 1 - int(rng.integers(0, max(1, n // 50)))
        bad[pos] ^= 1 << int(rng.integers(0, 8))
    else:
        t = int(rng.integers(1, 4))
        bad[n - t:] = bytes(t)
    return bytes(bad)


_CASES = {}


def decode_cases(chain, ent):
    """-> list of (tag, stream bytes, nbits, damaged?, oracle r, oracle bytes, original block): every block of the ragged set whole,
    then damaged in place.  Computed on the CPU alone."""
    key = (chain, ent)
    if key in _CASES:
        return _CASES[key]
    rng = np.random.default_rng(sum(map(ord, chain + ent)))
    out = []
    blocks = [b for b in _blocks() if len(b) > 0]
    refs = [_encode_ref(chain, ent, b) for b in blocks]
    for i, (b, (s, w, _, _)) in enumerate(zip(blocks, refs)):
        r, o = _decode_ref(chain, ent, s, w)
        assert r == len(b) and o == b, (chain, ent, len(b))          # the oracle's own round trip
        out.append(("whole %d" % len(b), s, w, False, r, o, b))
    for i, (b, (s, w, _, _)) in enumerate(zip(blocks, refs)):
        for j in range(2):
            bad = _damaged(rng, s, 2 * i + j)
            r, o = _decode_ref(chain, ent, bad, w)
            out.append(("damaged %d/%d" % (len(b), (2 * i + j) % 8), bad, w, True, r, o, b))
    _CASES[key] = out
    return out


def _decode_layouts(max_bytes, device):
    """(inStride, in base, outStride, out base): the tightest stride the contract allows, that + 1, that + 3 and the Java reader
    hook's kz_max_block_stream_bytes(bs) + 64, at base offsets 0, 1, 4, 64"""
    tight = max_bytes + (SLACK if device else 0)
    pad = max(512, BS >> 4)
    return [(tight, 0, BS, 0), (tight + 1, 1, BS + 1, 3), (tight + 3, 4, BS + pad, 1), (kz.max_block_stream_bytes(BS) + 64, 64, BS, 64)]


def _run_decode(ctx, chain, ent, cases, nbits, fill, layout, device, seed=0):
    """one kz_decode_blocks call over `cases` in a framed layout -> (results, output rows, input frame, output frame)"""
    in_stride, base, out_stride, obase = layout
    B = len(cases)
    fin = Frame(base + B * in_stride, fill, device, seed)
    for b, c in enumerate(cases):
        fin.put_stream(base + b * in_stride, c[1], int(nbits[b]))
    fout = Frame(obase + B * out_stride, fill, device, seed + 1)
    res = kz.decode_blocks(ctx, chain, ent, BS, fin.ptr(base), in_stride, nbits, fout.ptr(obase), out_stride,
                           kz.MEM_DEVICE if device else kz.MEM_HOST)
    return res, fout.rows(obase, out_stride, B, out_stride), fin, fout


def _check_decode(tag, cases, res, rows, fin, fout):
    acc = rej = 0
    for b, (what, s, w, damaged, r, o, orig) in enumerate(cases):
        ok = lh.check_decoded(tag + (b, what), res[b].status, res[b].length, rows[b], r, o)
        if not damaged:
            assert ok and bytes(rows[b][:len(orig)]) == orig, ("clean neighbour", tag, b, what)
        acc += ok
        rej += not ok
    lh.assert_guards(fout, tag + ("out",))
    assert fin.untouched(), ("input changed", tag)
    return acc, rej


@pytest.mark.parametrize("chain,ent", COMBOS)
def test_decode_ignores_everything_behind_the_stream(ctx, chain, ent):
    """Whole and damaged streams of one batch, device and host memory, four layouts x three fills: status, length and bytes of
    every block are the oracle's for that stream alone, whatever lies in the spare bits and behind."""
    ctx.set_block_size(BS)
    cases = decode_cases(chain, ent)
    nbits = np.array([c[2] for c in cases], dtype=np.int64)
    max_bytes = int((nbits.max() + 7) // 8)
    for device in (True, False):
        for li, layout in enumerate(_decode_layouts(max_bytes, device)):
            for fi, fill in enumerate(FILLS):
                if not device and (li + fi) % 2:                  # host memory: the fill is not what the device sees (next test)
                    continue
                res, rows, fin, fout = _run_decode(ctx, chain, ent, cases, nbits, fill, layout, device, seed=li)
                _check_decode((chain, ent, "device" if device else "host", layout, fill), cases, res, rows, fin, fout)


def _predecessor(ctx, chain, ent, B, kind):
    """leave the context's arena full of another batch's data: decode B long blocks of the same geometry"""
    rng = np.random.default_rng(kind)
    few = [bytes(rng.integers(0, 256, BS, dtype=np.uint8)) if kind == 0 else bytes([0xFF]) * 40000 + datagen.block(1, BS - 40000).tobytes() for _ in range(3)]
    refs = [_encode_ref(chain, ent, b) for b in few]
    cases = [("pred", refs[b % 3][0], refs[b % 3][1], False, BS, few[b % 3], few[b % 3]) for b in range(B)]
    nbits = np.array([c[2] for c in cases], dtype=np.int64)
    layout = _decode_layouts(int((nbits.max() + 7) // 8), False)[0]
    res, rows, fin, fout = _run_decode(ctx, chain, ent, cases, nbits, "zero", layout, False)
    _check_decode((chain, ent, "predecessor", kind), cases, res, rows, fin, fout)


@pytest.mark.parametrize("chain,ent", [("BWT+RANK+ZRLT", "ANS0"), ("LZ", "HUFFMAN"), ("BWT+SRT+ZRLT", "FPAQ"), ("ZRLT", "NONE")])
def test_host_decode_after_another_batch(ctx, chain, ent):
    """kz_decode_blocks copies (bits + 7) / 8 bytes of a host stream into an arena slot it does not clear: behind the stream lies
    whatever the previous call left there.  Two different predecessors, the same results."""
    cases = decode_cases(chain, ent)
    nbits = np.array([c[2] for c in cases], dtype=np.int64)
    layout = _decode_layouts(int((nbits.max() + 7) // 8), False)[0]
    for kind in (0, 1):
        _predecessor(ctx, chain, ent, len(cases), kind)
        res, rows, fin, fout = _run_decode(ctx, chain, ent, cases, nbits, "rand", layout, False)
        _check_decode((chain, ent, "host after", kind), cases, res, rows, fin, fout)


def test_decode_case_mix_is_not_one_sided():
    """the cap of the issue: per coder at least 10 of the compared block streams are ones the oracle accepts (bytes compared) and at
    least 30 ones it rejects -- over the damaged streams alone, the whole ones come on top"""
    tally = {}
    for chain, ent in COMBOS:
        a, r = tally.get(ent, (0, 0))
        for c in decode_cases(chain, ent):
            if c[3]:
                a += c[4] >= 0
                r += c[4] < 0
        tally[ent] = (a, r)
    print("damaged block streams accepted / rejected by the oracle:", tally)
    for ent, (a, r) in tally.items():
        assert a >= 10 and r >= 30, (ent, a, r)


@pytest.mark.parametrize("ent,chain", [("ANS0", "BWT+RANK+ZRLT"), ("HUFFMAN", "LZ"), ("FPAQ", "BWT+SRT+ZRLT"), ("NONE", "ZRLT"), ("ANS1", "NONE")])
def test_cut_bit_lengths_are_rejected_whatever_follows(ctx, ent, chain):
    """bitLengths[b] cut by 1, by 8 and to half: the frame check rejects the block (the header's checksum covers the bit length)
    and that does not depend on the bytes that now lie behind the cut -- the rest of the stream itself, then the fill."""
    blocks = [b for b in _blocks() if len(b) > 33][:6]
    refs = [_encode_ref(chain, ent, b) for b in blocks]
    cases, nbits = [], []
    for i, (b, (s, w, _, _)) in enumerate(zip(blocks, refs)):
        cut = (0, 1, 8, w // 2, 0, 1)[i]
        # the oracle's verdict on the cut stream (ANS1: the frame check precedes the coder, so ANS0's frame check is asked)
        r, o = _decode_ref(chain, ent if ent != "ANS1" else "ANS0", s, w - cut) if cut else (len(b), b)
        assert (r < 0) == (cut > 0)
        cases.append(("cut %d" % cut, s, w - cut, cut > 0, r, o, b))
        nbits.append(w - cut)
    nbits = np.array(nbits, dtype=np.int64)
    max_bytes = int((nbits.max() + 7) // 8)
    for device in (True, False):
        for li, layout in enumerate(_decode_layouts(max_bytes, device)[:2]):
            for fill in FILLS:
                res, rows, fin, fout = _run_decode(ctx, chain, ent, cases, nbits, fill, layout, device)
                _check_decode((chain, ent, device, layout, fill), cases, res, rows, fin, fout)


@pytest.mark.parametrize("chain", ANS1_CHAINS)
def test_ans1_decode_ignores_everything_behind_the_stream(ctx, chain):
    """ANS1 block streams written by the model: four layouts x three fills on the device, the arena's history on the host"""
    blocks = _blocks([16385, 17, 32768, 1, 40000, 15, 16, 65536, 33, 34], first=3)
    cases = []
    for b in blocks:
        s, w, _, _ = _encode_ref(chain, "ANS1", b)
        cases.append(("whole %d" % len(b), s, w, False, len(b), b, b))
    nbits = np.array([c[2] for c in cases], dtype=np.int64)
    max_bytes = int((nbits.max() + 7) // 8)
    for li, layout in enumerate(_decode_layouts(max_bytes, True)):
        for fill in FILLS:
            res, rows, fin, fout = _run_decode(ctx, chain, "ANS1", cases, nbits, fill, layout, True, seed=li)
            _check_decode((chain, "ANS1", layout, fill), cases, res, rows, fin, fout)
    layout = _decode_layouts(max_bytes, False)[1]
    for kind in (0, 1):
        _predecessor(ctx, chain, "ANS1", len(cases), kind)
        res, rows, fin, fout = _run_decode(ctx, chain, "ANS1", cases, nbits, "ones", layout, False)
        _check_decode((chain, "ANS1", "host after", kind), cases, res, rows, fin, fout)


@pytest.mark.parametrize("ent,chain", [("ANS0", "BWT+RANK+ZRLT"), ("HUFFMAN", "LZ"), ("FPAQ", "BWT+SRT+ZRLT"), ("NONE", "ZRLT"), ("ANS1", "NONE")])
def test_decode_one_4mib_block(ctx, ent, chain):
    """one 4 MiB block per coder, alone in its batch at the tightest stride: whole, and cut by one bit"""
    n = 1 << 22
    data = datagen.block(2, n).tobytes()
    s, w, _, _ = oracle.encode_block(chain, ent if ent != "ANS1" else "NONE", data, block_size=n)
    if ent == "ANS1":
        s, w = _ans1_block_from_none(s, w, n, len(chain.split("+")))
    r, o = oracle.decode_block(chain, ent if ent != "ANS1" else "ANS0", n, s, w - 1, n)
    assert r < 0
    ctx.set_block_size(n)
    try:
        for fill in FILLS:
            for cut, want_r in ((0, n), (1, r)):
                nby = (w - cut + 7) // 8
                fin = Frame(5 + nby + SLACK, fill, True)
                fin.put_stream(5, s, w - cut)
                fout = Frame(3 + n, fill, True, 1)
                res = kz.decode_blocks(ctx, chain, ent, n, fin.ptr(5), nby + SLACK, np.array([w - cut], dtype=np.int64), fout.ptr(3), n, kz.MEM_DEVICE)
                lh.check_decoded((chain, ent, fill, cut), res[0].status, res[0].length, fout.rows(3, n, 1, n)[0], want_r, data)
                lh.assert_guards(fout, (chain, ent, fill, cut))
    finally:
        ctx.set_block_size(BS)


# ---- kz_entropy_decode -----------------------------------------------------------------------------------------------------

def _model_decode(bits, nbits, count):
    try:
        r, out, used, _ = ans1model.decode(bits, nbits, count, 1)
    except katmodels.JavaException:
        return -1, b"", 0
    return r, out, used


def _entropy_ref(ent, stream, nbits, count):
    if ent == "ANS1":
        return _model_decode(stream[:(nbits + 7) // 8], nbits, count)
    return oracle.entropy_decode(ent, stream[:(nbits + 7) // 8], nbits, count)


_ECASES = {}


def entropy_cases(ent):
    """-> list of (tag, stream, inBits, count, oracle r, bytes, bits consumed): five inputs x eight bit lengths x four counts, then
    mild damage (one flip in the last 2 %, a short zeroed tail) of the whole streams until accepted and rejected cases are both
    plenty.  CPU only."""
    if ent in _ECASES:
        return _ECASES[ent]
    rng = np.random.default_rng(len(ent) * 7 + ord(ent[0]))
    sizes = (40, 300, 1000, 1500, 700) if ent == "ANS1" else (40, 1000, 40000, 16417, 5000)
    out = []
    for i, n in enumerate(sizes):
        data = datagen.block(i, n).tobytes()
        s, w = ans1model.encode(data, 1) if ent == "ANS1" else oracle.entropy_encode(ent, data)
        for cut in (0, 1, 3, 8, 9, 64, w - 3 * w // 4, w - w // 2):
            nb = w - cut
            if nb <= 0:
                continue
            for count in (n - 1, n, n + 1, 33):
                r, o, used = _entropy_ref(ent, s, nb, count)
                out.append(("%d bytes, %d of %d bits, count %d" % (n, nb, w, count), s, nb, count, r, o, used))
        for j in range(10):
            bad = bytearray(s)
            nby = (w + 7) // 8
            if j % 2:
                pos = nby - 1 - int(rng.integers(0, max(1, nby // 50)))
                bad[pos] ^= 1 << int(rng.integers(0, 8))
            else:
                t = int(rng.integers(1, 4))
                bad[nby - t:] = bytes(t)
            r, o, used = _entropy_ref(ent, bytes(bad), w, n)
            out.append(("%d bytes, mild damage %d" % (n, j), bytes(bad), w, n, r, o, used))
    _ECASES[ent] = out
    return out


@pytest.mark.parametrize("ent", ["ANS0", "HUFFMAN", "FPAQ", "NONE", "ANS1"])
def test_entropy_decode_ignores_spare_bits_and_tail(ctx, ent):
    """kz_entropy_decode with the fill in the spare bits of the last byte and behind (inBits + 7) / 8 of the host array: verdict,
    bytes and bits consumed equal the oracle's (ANS1: the model's) under every fill.  At least 10 accepted and 30 rejected cases."""
    cases = entropy_cases(ent)
    acc = rej = 0
    for tag, s, nb, count, r, o, used in cases:
        for fi, fill in enumerate(FILLS):
            fin = Frame((nb + 7) // 8, fill, False, seed=fi, guard=1024)
            fin.put_stream(0, s, nb)
            fout = Frame(count, fill, False, seed=fi + 1, guard=1024)
            u = ctypes.c_int64(-1)
            rc = ctx.lib.kz_entropy_decode(ctx.h, kz.ENTROPY_IDS[ent], fin.ptr(0), nb, fout.ptr(0), count, ctypes.addressof(u))
            ok = lh.check_entropy_decoded((ent, tag, fill), rc, fout.rows(0, count, 1, count)[0], u.value, count, r, o, used)
            lh.assert_guards(fout, (ent, tag, fill))
            assert fin.untouched()
        acc += ok
        rej += not ok
    print("entropy cases accepted / rejected by the reference:", ent, acc, rej)
    assert acc >= 10 and rej >= 30, (ent, acc, rej)


# ---- encode ----------------------------------------------------------------------------------------------------------------

ENC_COMBOS = COMBOS + [("DNA+LZ", "HUFFMAN")] + [(c, "ANS1") for c in ANS1_CHAINS]
_EREFS = {}


def encode_refs(chain, ent, blocks_key="ragged"):
    key = (chain, ent, blocks_key)
    if key not in _EREFS:
        blocks = _blocks() if blocks_key == "ragged" else _blocks(first=7)
        if chain.startswith("DNA"):                        # something DNA packs: the ragged lengths of an ACGT text
            acgt = dict(refinputs.alias_inputs())["acgt+0"]
            blocks = [acgt[i * 11:i * 11 + len(b)] if i % 2 else b for i, b in enumerate(blocks)]
        _EREFS[key] = (blocks, [_encode_ref(chain, ent, b) for b in blocks])
    return _EREFS[key]


def _encode_layouts(max_len):
    """(inStride, in base, outStride, out base): device input at maxLen, + 1, + 13, x 2 and bases 0, 1, 3; device output at
    need, + 4, + 12, + 260 and the 4-aligned bases 0, 4, 60"""
    need = kz.max_block_stream_bytes(max_len)
    return [(max_len, 0, need, 0), (max_len + 1, 1, need + 4, 4), (max_len + 13, 3, need + 12, 60), (2 * max_len, 1, need + 260, 4)]


def _run_encode(ctx, chain, ent, blocks, fill, layout, device, seed=0, call=None):
    in_stride, base, out_stride, obase = layout
    B = len(blocks)
    lens = np.array([len(b) for b in blocks], dtype=np.int32)
    fin = Frame(base + (B - 1) * in_stride + int(lens.max()), fill, device, seed)
    for b, blk in enumerate(blocks):
        fin.put(base + b * in_stride, blk)
    fout = Frame(obase + B * out_stride, fill, device, seed + 1)
    call = call or kz.encode_blocks
    res = call(ctx, chain, ent, fin.ptr(base), in_stride, lens, fout.ptr(obase), out_stride, kz.MEM_DEVICE if device else kz.MEM_HOST)
    return res, fin, fout, (obase, out_stride, B)


def _check_encode(tag, refs, res, fin, fout, geo):
    obase, out_stride, B = geo
    rows = fout.rows(obase, out_stride, B, out_stride)
    for b in range(B):
        lh.check_stream(tag + (b,), res[b], rows[b], refs[b])
    lh.assert_guards(fout, tag)
    assert fin.untouched(), ("input changed", tag)
    return rows


@pytest.mark.parametrize("chain,ent", ENC_COMBOS)
def test_encode_depends_on_the_block_alone(ctx, chain, ent):
    """Ragged batches (lengths 0, 1, 15, 16, 32, 33 in the middle) in device memory, the gaps between the blocks and the output
    frame taken from the fill: stream bytes, bits, length, skipFlags and mode of every block equal oracle.encode_block of that
    block alone, in every layout and under every fill; nothing outside out[0 .. nBlocks * outStride) is written."""
    ctx.set_block_size(BS)
    blocks, refs = encode_refs(chain, ent)
    layouts = _encode_layouts(max(len(b) for b in blocks))
    for i in range(6):
        layout, fill = layouts[i % 4], FILLS[i % 3]
        res, fin, fout, geo = _run_encode(ctx, chain, ent, blocks, fill, layout, True, seed=i)
        _check_encode((chain, ent, layout, fill), refs, res, fin, fout, geo)
    # B == 1 (a block alone, at an odd address), and host memory with the output guard behind the last row
    for b in (0, 5, 8):
        l1 = _encode_layouts(len(blocks[b]))[2]
        res, fin, fout, geo = _run_encode(ctx, chain, ent, [blocks[b]], "rand", l1, True, seed=b)
        _check_encode((chain, ent, "alone", b), [refs[b]], res, fin, fout, geo)
    res, fin, fout, geo = _run_encode(ctx, chain, ent, blocks, "ones", layouts[1], False)
    _check_encode((chain, ent, "host"), refs, res, fin, fout, geo)


def test_encode_refuses_what_the_contract_forbids(ctx):
    """device `out` at a base offset of 1 or 2, an outStride of need + 2 or below need, an inStride below the longest block:
    -KZ_ERR_INVALID_PARAM before anything is launched, the whole output frame untouched; and nBlocks == 0 returns 0 and writes
    nothing.  (The forbidden layouts never reach a kernel.)"""
    blocks, _ = encode_refs("LZ", "HUFFMAN")
    max_len = max(len(b) for b in blocks)
    need = kz.max_block_stream_bytes(max_len)
    for device in (True, False):
        bad = [(max_len, 0, need + 2, 0), (max_len, 0, need - 4, 0), (max_len - 1, 0, need, 0)]
        if device:
            bad += [(max_len, 0, need, 1), (max_len, 0, need + 4, 2), (max_len + 1, 1, need, 3)]
        for layout in bad:
            caught = {}

            def call(*a):
                try:
                    return kz.encode_blocks(*a)
                except kz.KanziError as e:
                    caught["code"] = e.code
                    return None
            res, fin, fout, geo = _run_encode(ctx, "LZ", "HUFFMAN", blocks, "rand", layout, device, call=call)
            assert caught.get("code") == 18, (layout, device, caught)
            assert fout.untouched() and fin.untouched(), (layout, device)
        fout = Frame(need, "rand", device)
        fin = Frame(max_len, "rand", device)
        res = kz.encode_blocks(ctx, "LZ", "HUFFMAN", fin.ptr(0), max_len, np.zeros(0, dtype=np.int32), fout.ptr(0), need, kz.MEM_DEVICE if device else kz.MEM_HOST)
        assert len(res) == 0 and fout.untouched()


def test_decode_refuses_what_the_contract_forbids(ctx):
    """a device slot without KZ_STREAM_SLACK bytes behind its stream, host slots shorter than their streams, a negative bit
    length: -KZ_ERR_INVALID_PARAM, output untouched; nBlocks == 0 returns 0"""
    cases = decode_cases("LZ", "HUFFMAN")[:4]
    nbits = np.array([c[2] for c in cases], dtype=np.int64)
    max_bytes = int((nbits.max() + 7) // 8)
    for device, stride, nb in ((True, max_bytes + SLACK - 1, nbits), (True, max_bytes, nbits), (False, max_bytes - 1, nbits),
                               (True, max_bytes + SLACK, np.array([nbits[0], -1, nbits[2], nbits[3]], dtype=np.int64))):
        B = len(cases)
        fin = Frame(B * (max_bytes + SLACK), "rand", device)
        fout = Frame(B * BS, "rand", device, 1)
        with pytest.raises(kz.KanziError) as e:
            kz.decode_blocks(ctx, "LZ", "HUFFMAN", BS, fin.ptr(0), stride, nb, fout.ptr(0), BS, kz.MEM_DEVICE if device else kz.MEM_HOST)
        assert e.value.code == 18, (device, stride)
        assert fout.untouched()
    fout = Frame(BS, "rand", True)
    fin = Frame(BS, "rand", True)
    assert len(kz.decode_blocks(ctx, "LZ", "HUFFMAN", BS, fin.ptr(0), BS, np.zeros(0, dtype=np.int64), fout.ptr(0), BS, kz.MEM_DEVICE)) == 0
    assert fout.untouched()


@pytest.mark.parametrize("chain,ent", [("BWT+RANK+ZRLT", "ANS0"), ("LZ", "HUFFMAN"), ("BWT+SRT+ZRLT", "FPAQ"), ("PACK+MM+LZX", "HUFFMAN"), ("NONE", "ANS1")])
def test_encode_does_not_depend_on_the_arenas_history(ctx, chain, ent):
    """The rows of the library's batch buffer behind lengths[b] are stale arena and kernels read past a block's end on purpose.
    The same host batch (i) on a fresh context, (ii) after a batch of full-length 0xFF blocks, (iii) after random blocks of twice
    the length: all equal the oracle.  Additional checks: a permuted batch, and one block moved between a batch of 1 and a batch
    of 64, give the same streams."""
    blocks, refs = encode_refs(chain, ent)
    B = len(blocks)
    max_len = max(len(b) for b in blocks)
    layout = _encode_layouts(max_len)[1]
    rng = np.random.default_rng(5)
    fresh = kz.Context(0)
    try:
        fresh.set_block_size(BS)
        res, fin, fout, geo = _run_encode(fresh, chain, ent, blocks, "rand", layout, False)
        _check_encode((chain, ent, "fresh context"), refs, res, fin, fout, geo)
        for what, prev in (("after 0xFF", [bytes([0xFF]) * max_len] * B), ("after random x 2", [bytes(rng.integers(0, 256, 2 * max_len, dtype=np.uint8))] * B)):
            _run_encode(fresh, chain, ent, prev, "zero", _encode_layouts(len(prev[0]))[0], False)
            res, fin, fout, geo = _run_encode(fresh, chain, ent, blocks, "rand", layout, False)
            _check_encode((chain, ent, what), refs, res, fin, fout, geo)
        perm = [int(x) for x in rng.permutation(B)]
        res, fin, fout, geo = _run_encode(fresh, chain, ent, [blocks[p] for p in perm], "ones", layout, True)
        _check_encode((chain, ent, "permuted"), [refs[p] for p in perm], res, fin, fout, geo)
        one = 8                                                     # the 65 536-byte block, alone and as row 37 of 64
        many = [blocks[(7 * i) % B] for i in range(64)]
        many[37] = blocks[one]
        res, fin, fout, geo = _run_encode(fresh, chain, ent, many, "rand", layout, True)
        _check_encode((chain, ent, "64"), [refs[(7 * i) % B] if i != 37 else refs[one] for i in range(64)], res, fin, fout, geo)
        res, fin, fout, geo = _run_encode(fresh, chain, ent, [blocks[one]], "rand", layout, True)
        _check_encode((chain, ent, "1"), [refs[one]], res, fin, fout, geo)
    finally:
        fresh.close()


def test_sync_submit_and_two_contexts_agree(ctx):
    """the synchronous call, kz_submit_* and a second context give the oracle's bytes on one non-trivial layout"""
    chain, ent = "BWT+RANK+ZRLT", "ANS0"
    blocks, refs = encode_refs(chain, ent)
    layout = _encode_layouts(max(len(b) for b in blocks))[2]
    other = kz.Context(0)
    try:
        for who, call in ((ctx, kz.encode_blocks), (ctx, lambda *a: kz.submit_encode_blocks(*a).wait()), (other, kz.encode_blocks),
                          (other, lambda *a: kz.submit_encode_blocks(*a).wait())):
            for device in (True, False):
                res, fin, fout, geo = _run_encode(who, chain, ent, blocks, "rand", layout, device, call=call)
                _check_encode((chain, ent, who is other, device), refs, res, fin, fout, geo)
        # both contexts in flight at once, then the decode the same way
        frames = [_run_encode(c, chain, ent, blocks, "ones", layout, True, call=kz.submit_encode_blocks) for c in (ctx, other)]
        for job, fin, fout, geo in frames:
            _check_encode((chain, ent, "overlapped"), refs, job.wait(), fin, fout, geo)
        cases = decode_cases(chain, ent)
        nbits = np.array([c[2] for c in cases], dtype=np.int64)
        dl = _decode_layouts(int((nbits.max() + 7) // 8), True)[1]
        B = len(cases)
        jobs = []
        for c in (ctx, other):
            fin = Frame(dl[1] + B * dl[0], "rand", True)
            for b, cs in enumerate(cases):
                fin.put_stream(dl[1] + b * dl[0], cs[1], int(nbits[b]))
            fout = Frame(dl[3] + B * dl[2], "rand", True, 1)
            jobs.append((kz.submit_decode_blocks(c, chain, ent, BS, fin.ptr(dl[1]), dl[0], nbits, fout.ptr(dl[3]), dl[2], kz.MEM_DEVICE), fin, fout))
        for job, fin, fout in jobs:
            _check_decode((chain, ent, "overlapped decode"), cases, job.wait(), fout.rows(dl[3], dl[2], B, dl[2]), fin, fout)
    finally:
        other.close()


# ---- more blocks than one launch ------------------------------------------------------------------------------------------

KB = 1024
MAX_BATCH = 65535                              # KZ_MAX_BATCH of kanzi_amd/csrc/kz_internal.h
_BIG = {}


def many_blocks(n):
    """n blocks of 1 KiB cut from five class buffers (class = b mod 5), every 97th shorter, a few of length 0 and 15"""
    if "src" not in _BIG:
        _BIG["src"] = [datagen.block(c, 1 << 20) for c in range(5)]
    src = _BIG["src"]
    lens = np.full(n, KB, dtype=np.int32)
    lens[::97] = KB - 1 - (np.arange(0, n, 97) % 89)
    for b in (5, 1000, MAX_BATCH - 1, MAX_BATCH, 2 * MAX_BATCH - 1, n - 1):
        if b < n:
            lens[b] = 0 if b % 2 else 15
    blocks = [src[b % 5][(b * 977) % ((1 << 20) - KB):][:lens[b]].tobytes() for b in range(n)]
    return blocks, lens


def many_refs(chain, ent, n):
    key = (chain, ent)
    if key not in _BIG or len(_BIG[key]) < n:
        blocks, _ = many_blocks(n)
        _BIG[key] = lh.oracle_map(lambda b: oracle.encode_block(chain, ent, b, block_size=KB), blocks)
    return _BIG[key][:n]


def _boundary_message(b, n):
    splits = [s for s in range(MAX_BATCH, n, MAX_BATCH)]
    near = [s for s in splits if abs(b - s) <= 1 or b == s - 1]
    return "block %d of %d (KZ_MAX_BATCH boundaries: blocks %s | %s)" % (b, n, [s - 1 for s in splits], splits) + (" AT A BOUNDARY" if near else "")


@pytest.mark.parametrize("chain,ent", [("BWT+RANK+ZRLT", "ANS0"), ("LZ", "HUFFMAN")])
@pytest.mark.parametrize("n", [MAX_BATCH + 2, 2 * MAX_BATCH + 1])
def test_more_blocks_than_one_launch(ctx, chain, ent, n):
    """nBlocks > KZ_MAX_BATCH: the calls recurse over sub-batches with pointer arithmetic on in, out, lengths and results.  Every
    block's result and stream equal the oracle's, the decode of the oracle's streams restores the input, output guards intact,
    device and host memory.  (The scratch arena's budget may split a batch EARLIER than at 65 535 blocks on a given
    machine -- chains with BWT leave half the arena to the suffix sort; the counts here stay as they are: the pointer arithmetic of
    the recursion is the same, it crosses block 65 535 either way, and the boundaries named in a failure are the KZ_MAX_BATCH ones.)"""
    ctx.set_block_size(KB)
    blocks, lens = many_blocks(n)
    refs = many_refs(chain, ent, n)
    need = kz.max_block_stream_bytes(KB)
    wbits = np.array([r[1] for r in refs], dtype=np.int64)
    wby = (wbits + 7) // 8
    for device in (True, False):
        mem = kz.MEM_DEVICE if device else kz.MEM_HOST
        # ---- encode ----
        fin = Frame(3 + n * KB, "ones", device)
        img = fin.img[fin.guard + 3:fin.guard + 3 + n * KB].reshape(n, KB)
        for b, blk in enumerate(blocks):
            if lens[b]:
                img[b, :lens[b]] = np.frombuffer(blk, dtype=np.uint8)
        fout = Frame(4 + n * need, "ones", device, 1)
        res = kz.encode_blocks(ctx, chain, ent, fin.ptr(3), KB, lens, fout.ptr(4), need, mem)
        after = fout.after()
        lh.assert_guards(fout, (chain, ent, n, device), after)
        rows = after[fout.guard + 4:fout.guard + 4 + n * need].reshape(n, need)
        got = np.array([(r.bits, r.length, r.status) for r in res], dtype=np.int64)
        want = np.array([(r[1], r[3], 0) for r in refs], dtype=np.int64)
        for b in np.nonzero((got != want).any(axis=1))[0][:3]:
            raise AssertionError(("bits / length / status", chain, ent, device, _boundary_message(int(b), n), got[b].tolist(), want[b].tolist()))
        for b in range(n):
            if rows[b, :wby[b]].tobytes() != refs[b][0]:
                raise AssertionError(("stream bytes", chain, ent, device, _boundary_message(b, n)))
        for b in (0, MAX_BATCH - 1, MAX_BATCH, MAX_BATCH + 1, n - 1):
            lh.check_stream((chain, ent, device, _boundary_message(b, n)), res[b], rows[b], refs[b])
        del after, rows, fout, fin
        # ---- decode the oracle's streams ----
        stride = int(wby.max()) + SLACK + 1
        fin = Frame(1 + n * stride, "ones", device)
        for b in range(n):
            fin.put_stream(1 + b * stride, refs[b][0], int(wbits[b]))
        fout = Frame(5 + n * (KB + 1), "ones", device, 1)
        res = kz.decode_blocks(ctx, chain, ent, KB, fin.ptr(1), stride, wbits, fout.ptr(5), KB + 1, mem)
        after = fout.after()
        lh.assert_guards(fout, (chain, ent, n, device, "decode"), after)
        rows = after[fout.guard + 5:fout.guard + 5 + n * (KB + 1)].reshape(n, KB + 1)
        for b in range(n):
            if res[b].status != 0 or res[b].length != lens[b] or rows[b, :lens[b]].tobytes() != blocks[b]:
                raise AssertionError(("decode", chain, ent, device, _boundary_message(b, n), res[b].status, res[b].length, int(lens[b])))
        del after, rows, fout, fin
    ctx.set_block_size(BS)


# ---- the one-block mirrors -------------------------------------------------------------------------------------------------

def _mirror_inputs(name=None):
    ins = refinputs.edge_inputs() + [datagen.block(c, 50000).tobytes() for c in range(5)]
    if name in ("PACK", "DNA"):
        ins += [d[:40001] for _, d in refinputs.alias_inputs()[:8]]
    if name in ("TEXT", "UTF"):
        ins += [bytes(textgen.english(30000, 1)), bytes(textgen.utf8(30000, 2)), bytes(textgen.xml(20001, 3))]
    if name == "MM":
        ins += [refinputs.multimedia_like(k, 40000 + k) for k in range(3)]
    return ins


def _call_transform(ctx, name, inverse, data, cap, fill):
    """kz_transform_* / kz_host_stage_* with dst = exactly `cap` bytes and a guard behind -> (rc, bytes produced, frame)"""
    tid = kz.TRANSFORM_IDS[name]
    src = np.frombuffer(data, dtype=np.uint8) if len(data) else np.zeros(1, dtype=np.uint8)
    dst = Frame(cap, fill, False, guard=4096)
    p = ctypes.c_int32(0)
    if name in ("TEXT", "UTF"):
        if inverse:
            rc = ctx.lib.kz_host_stage_inverse(tid, BS, src.ctypes.data, len(data), dst.ptr(0), cap, ctypes.addressof(p))
        else:
            dt = ctypes.c_int32(0)
            rc = ctx.lib.kz_host_stage_forward(tid, kz.E_NONE, BS, ctypes.addressof(dt), src.ctypes.data, len(data), dst.ptr(0), cap, ctypes.addressof(p))
    else:
        ctx.set_data_type(0)
        fn = ctx.lib.kz_transform_inverse if inverse else ctx.lib.kz_transform_forward
        rc = fn(ctx.h, tid, src.ctypes.data, len(data), dst.ptr(0), cap, ctypes.addressof(p))
    return rc, bytes(dst.rows(0, cap, 1, cap)[0][:p.value]) if rc == 1 else b"", dst


@pytest.mark.parametrize("name", ["BWT", "RANK", "MTFT", "SRT", "ZRLT", "LZ", "LZX", "MM", "PACK", "DNA", "TEXT", "UTF"])
def test_one_block_transforms_stay_inside_dst(ctx, name):
    """forward at exactly kz_transform_max_encoded_len, inverse at exactly the decoded length and at one byte more: the result is
    the oracle's, nothing behind dstCap is written, and a declined forward leaves dst untouched as the header promises"""
    oracle.set_transform_ctx("NONE", BS)
    ctx.set_entropy("NONE")
    ctx.set_block_size(BS)
    applied = 0
    for i, data in enumerate(_mirror_inputs(name)):
        fill = FILLS[i % 3]
        ok_o, enc_o, _ = oracle.transform_forward(name, data, data_type=0)
        cap = int(ctx.lib.kz_transform_max_encoded_len(kz.TRANSFORM_IDS[name], len(data)))
        rc, enc, dst = _call_transform(ctx, name, False, data, cap, fill)
        assert rc == (1 if ok_o else 0), (name, len(data), rc, ctx.error())
        lh.assert_guards(dst, (name, "forward", len(data)))
        if not ok_o:
            assert dst.untouched(), (name, "declined forward wrote to dst", len(data))
            continue
        applied += 1
        assert enc == enc_o, (name, "forward", len(data))
        for extra in (0, 1):
            ok_i, back_o = oracle.transform_inverse(name, enc_o, len(data) + extra)
            rc, back, dst = _call_transform(ctx, name, True, enc_o, len(data) + extra, fill)
            assert rc == (1 if ok_i else 0), (name, "inverse", len(data), extra, rc, ok_i)
            if ok_i:
                assert back == back_o == data, (name, "inverse", len(data), extra)
            lh.assert_guards(dst, (name, "inverse", len(data), extra))
    ctx.set_data_type(0)
    assert applied >= 1, (name, applied)


@pytest.mark.parametrize("ent", ["ANS0", "HUFFMAN", "FPAQ", "NONE", "ANS1"])
def test_entropy_encode_stays_inside_out(ctx, ent):
    """kz_entropy_encode with a guard behind outCapBytes: the oracle's (ANS1: the model's) bits, the guard intact"""
    for i, data in enumerate(_mirror_inputs()):
        if ent == "ANS1" and len(data) > 20000:
            data = data[:20000]
        want, wbits = ans1model.encode(data, 1) if ent == "ANS1" else oracle.entropy_encode(ent, data)
        cap = kz.max_block_stream_bytes(len(data)) + (102400 if ent == "ANS1" else 0)
        out = Frame(cap, FILLS[i % 3], False, guard=4096)
        src = np.frombuffer(data, dtype=np.uint8)
        nbits = ctx.lib.kz_entropy_encode(ctx.h, kz.ENTROPY_IDS[ent], src.ctypes.data, len(data), out.ptr(0), cap)
        assert nbits == wbits, (ent, len(data), nbits, wbits)
        assert bytes(out.rows(0, cap, 1, cap)[0][:(wbits + 7) // 8]) == want, (ent, len(data))
        lh.assert_guards(out, (ent, len(data)))
