"""Every transform taken alone crossed with every entropy coder, replayed byte for byte against tests/golden/codec_grid.json, which
tools/codec_grid.py recorded on the GPU at the commit before the transforms and coders were dispatched from one table each: the
batched calls' streams and block results, the single-block calls' bytes and return values, and what ids outside the tables get."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import codec_grid as G

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded():
    with open(G.FIXTURE) as f:
        return json.load(f)


def test_fixture_covers_the_grid(recorded):
    """15 transforms x 7 coders, five blocks each, and every transform applied somewhere: a stage that never ran would pass"""
    assert sorted(recorded["cells"]) == sorted("%s&%s" % (t, e) for t in G.TRANSFORMS for e in G.ENTROPIES)
    assert len(G.TRANSFORMS) == 15 and len(G.ENTROPIES) == 7 and len(recorded["cells"]) == 105
    assert all(len(c) == len(G.LENGTHS) for c in recorded["cells"].values())
    assert G.never_applied(recorded) == []
    assert all(r["restored"] for c in recorded["cells"].values() for r in c if r["status"] == 0)
    assert sorted(recorded["transforms"]) == sorted(G.TRANSFORMS) and sorted(recorded["entropies"]) == sorted(G.ENTROPIES)
    # the single-block calls: every coder and every transform coded a block and gave it back
    assert all(r["encode"] > 0 and r["decode"] == 1500 and r["restored"] for r in recorded["entropies"].values())
    for t, r in recorded["transforms"].items():
        r = r.get("block_70000", r)                                        # the block the stage applied to
        assert r["forward"] == 1 and r["inverse"] == 1 and r["restored"], t


@pytest.mark.parametrize("entropy", G.ENTROPIES)
def test_batched_calls(ctx, recorded, entropy):
    for t in G.TRANSFORMS:
        key = "%s&%s" % (t, entropy)
        got = G.cell(ctx, t, entropy)
        for i, (w, g) in enumerate(zip(recorded["cells"][key], got)):
            assert g == w, (key, "block of %d bytes" % G.LENGTHS[i], g, w)
    ctx.reset()


def test_single_block_calls(ctx, recorded):
    for t in G.TRANSFORMS:
        assert G.single_transform(ctx, t) == recorded["transforms"][t], t
    for e in G.ENTROPIES:
        assert G.single_entropy(ctx, e) == recorded["entropies"][e], e
    ctx.reset()


def test_ids_outside_the_tables(ctx):
    """ERR_INVALID_CODEC from the batched and the single-block calls for every id that has no row, the batched call naming the id;
    never for an id that has one (but NONE as a single transform: there is no stage to run, kz_transform_forward refuses it)"""
    outside, inside = G.unknown_ids(ctx)
    assert len(outside) == 2 * (64 - 16) + 2 * (16 - 7) and len(inside) == 2 * 16 + 2 * 7
    for call, i, rc, err in outside:
        assert rc == -3, (call, i, rc)
        if call == "kz_encode_blocks transform":
            assert err == "unsupported transform id %d" % i
        if call == "kz_encode_blocks entropy":
            assert err == "unsupported entropy id %d" % i
    for call, i, rc, err in inside:
        assert (rc == -3) == ((call, i) == ("kz_transform_forward", 0)), (call, i, rc, err)
