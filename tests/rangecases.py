"""Inputs and expected results shared by tests/test_range_model.py (no GPU) and tests/test_gpu_range.py: the single-block parity
inputs, the input that reaches the encoder's low-range branch, streams the encoder never writes, and the damaged-stream set with
the model's verdicts.  Everything expensive is computed once per process."""
import functools

import numpy as np

import datagen
import katmodels
import rangemodel
import refinputs

CHUNK = 1 << 15
# lr thresholds (256, 512, 4096), one chunk, the one-byte tail chunk (lr 8, one symbol), second-chunk and three-chunk seams
SEAM_LENGTHS = (0, 1, 2, 255, 256, 257, 511, 512, 4095, 4096, 32767, 32768, 32769, 32768 + 256, 3 * 32768 + 5)


@functools.lru_cache(maxsize=None)
def low_range_input():
    """chunks 14 and 15 of a fixed random megabyte: the encoder takes `range = -low & 0xFFFF` once in each"""
    return np.random.default_rng(1).integers(0, 256, 1 << 20, dtype=np.uint8)[14 << 15:16 << 15].tobytes()


@functools.lru_cache(maxsize=None)
def many_chunks_input():
    """65 chunks + 1 byte (the chunk scan past one wave's width).  Most chunks are one repeated byte (header only, cheap in the
    model); chunks 0, 31, 63 and 64 are coded."""
    parts = []
    for c in range(65):
        parts.append(datagen.block(c % 5, CHUNK).tobytes() if c in (0, 31, 63, 64) else bytes([c + 1]) * CHUNK)
    return b"".join(parts) + b"\x07"


@functools.lru_cache(maxsize=None)
def parity_inputs():
    """[(label, bytes)]: every input of the single-block parity test"""
    rng = np.random.default_rng(5)
    out = [("entropy%d" % i, d) for i, d in enumerate(refinputs.entropy_inputs())]
    out += [("edge%d" % i, d) for i, d in enumerate(refinputs.edge_inputs())]
    for n in SEAM_LENGTHS:
        out.append(("skewed%d" % n, bytes(np.minimum(rng.geometric(0.2, n) - 1, 255).astype(np.uint8))))
    text = datagen.block(3, CHUNK).tobytes()
    out.append(("skipped middle chunk", text + b"\x55" * CHUNK + datagen.block(0, 5000).tobytes()))
    out.append(("one byte value", b"\xAA" * (2 * CHUNK + 77)))
    out.append(("low range", low_range_input()))
    out.append(("65 chunks + 1", many_chunks_input()))
    return out


def model_decode(bits, nbits, count):
    """-> (ok, bytes, bits consumed) of the reference's decoder; ok False where it throws or returns another count"""
    try:
        r, out, used = rangemodel.decode(bits, nbits, count)
    except katmodels.JavaException:
        return False, None, None
    return r == count, out, used


def _chunk_tables(chunk, lr):
    """(header bits, cumulative frequencies) the encoder gives a chunk at lr"""
    freqs = [0] * 256
    for b in chunk:
        freqs[b] += 1
    alphabet = katmodels._normalize(freqs, len(chunk), 1 << lr)
    bs = rangemodel._Bits()
    rangemodel.encode_header(bs, alphabet, freqs, lr)
    cum = [0]
    for f in freqs:
        cum.append(cum[-1] + f)
    return bs.n, cum


@functools.lru_cache(maxsize=None)
def unusual_streams():
    """[(label, bits, nbits, count, model verdict)]: streams the encoder never writes.  lr 8, 9 and 15 for the whole block, and
    streams stitched from a chunk at lr 15 followed by one at lr 8: f2s only grows (RangeDecoder.java:226-227), so the second chunk's
    table is the first 256 entries of a 32 768-entry array whose rest is the first chunk's.  A 60-bit code of all ones makes the second
    chunk's first quotient (2^60 - 1) / (2^52 - 1) = 256: the entry the first chunk left at index 256, symbol `stale`.  In one
    stream the second chunk does not have that symbol (frequency 0: range becomes 0 and the loop never ends), in the other it does."""
    rng = np.random.default_rng(8)
    text = datagen.block(3, CHUNK).tobytes()
    cum15 = _chunk_tables(text, 15)[1]
    stale = max(i for i in range(256) if cum15[i] <= 256)
    others = [b for b in range(97, 105) if b != stale][:7]
    tails = {"absent": bytes(rng.choice(others, 3000).astype(np.uint8)),
             "present": bytes(rng.choice(others[:6] + [stale], 3000).astype(np.uint8))}
    data = text + tails["absent"]
    out = []
    for lr in (8, 9, 15):
        bits, nbits = rangemodel.encode(data, lr=lr)
        out.append(("lr %d" % lr, bits, nbits, len(data), model_decode(bits, nbits, len(data))))
    for kind, tail in tails.items():
        bs = rangemodel._Bits()
        rangemodel.encode_chunk(bs, text, 15)
        n0 = bs.n
        rangemodel.encode_chunk(bs, tail, 8)
        bits, nbits, count = bs.bytes(), bs.n, CHUNK + len(tail)
        if kind == "absent":
            out.append(("lr 15 then 8", bits, nbits, count, model_decode(bits, nbits, count)))
        bad = bytearray(bits)
        refinputs.set_bits(bad, n0 + _chunk_tables(tail, 8)[0], 60, (1 << 60) - 1)
        verdict = model_decode(bytes(bad), nbits, count)
        assert rangemodel.stale_reads[0] >= 1
        out.append(("stale symbol %s" % kind, bytes(bad), nbits, count, verdict))
    return out


@functools.lru_cache(maxsize=None)
def damaged_trials():
    """[(class, trial, bits, nbits, count, model verdict)]: two data classes x 24 refinputs.corrupt trials"""
    rng = np.random.default_rng(99)
    out = []
    for cls in (0, 3):
        data = datagen.block(cls, 40000).tobytes()
        good, nbits = rangemodel.encode(data)
        for trial in range(24):
            bad = refinputs.corrupt(rng, good, trial % 8)
            nb = min(nbits, len(bad) * 8)
            out.append((cls, trial, bad, nb, len(data), model_decode(bad, nb, len(data))))
    return out
