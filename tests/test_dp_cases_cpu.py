"""What makes test_gpu_dp_geometries.py's comparison meaningful, checked on the oracle alone (CPU only): properties of dp_cases.py's
inputs, not measurements of the code under test.  Every batch's longest read is exactly its geometry's `hi`, so that pick_geom's rule
(dp_cases.PICK_GEOM, which the GPU test holds against pemap_dev_sw_geom) puts it where it is meant to run; the planted seam gaps are
found as gaps; every read length maps; windows of unequal height, ends with several hits and windows with odd letters occur in numbers.
A generator that misses a floor is to be mended; the floors stay."""
import functools

import numpy as np
import pytest

import dp_cases as dc
import oracle_py

GI = list(range(len(dc.GEOMS)))
IDS = [dc.geom_name(g) for g in GI]


@functools.lru_cache(maxsize=None)
def _oracle(gi, name):
    """the oracle's results for one batch on an empty pileup (computed once, never modified)"""
    paired, reads, meta = dc.batches(gi)[name]
    o = oracle_py.Oracle(dc.index(), paired=paired, **dc.PARAMS)
    m1, m2, mt, d1, d2 = o.map_batch(*reads, debug=True, threads=8)
    return dict(m1=m1, m2=m2, mt=mt, d=(d1, d2), dels=int(o.counts()[:, 4].astype(np.int64).sum()), n_ins=len(o.insertions()))


def _subject(r, first):
    """per pair, of the end that the generator made on purpose (read 1 where `first`): mapped coordinate and debug record index"""
    return np.where(first, r["m1"], r["m2"])


def _gapped_alignments(reads, r):
    """single-hit mapped ends whose DP score beats every diagonal of the window: their alignment holds a gap (letters A, C, G, T only)"""
    genome = dc.index()["genome"]
    n = 0
    for which in (0, 1):
        d, m = r["d"][which], (r["m1"], r["m2"])[which]
        rows, lens = reads[2 * which], reads[2 * which + 1]
        for i in np.nonzero((d["n_hits"] == 1) & (m > 0))[0]:
            mm, ws, wl = int(lens[i]), int(d["win_start"][i, 0]), int(d["win_len"][i, 0])
            if wl < mm:
                continue
            q = rows[i, :mm]
            if d["orient"][i, 0]:
                q = dc.COMP[q][::-1]
            w = genome[ws:ws + wl]
            eq = max(int((w[k:k + mm] == q).sum()) for k in range(wl - mm + 1))
            n += d["score"][i, 0] > eq - (mm - eq) / 3 + 1e-6
    return int(n)


@pytest.mark.parametrize("gi", GI, ids=IDS)
def test_longest_read_selects_the_geometry(gi):
    lanes, W, hi = dc.GEOMS[gi]
    assert lanes * W >= hi and dc.picked(hi, gapless_on=False) == (lanes, W)
    assert dc.picked(hi) == ((16, 10) if (lanes, W) == (8, 19) else (lanes, W))
    # the table is pick_geom's: contiguous over the supported lengths, the smallest listed form that holds the read
    assert dc.PICK_GEOM[0][0] == 16 and dc.PICK_GEOM[-1][1] == 278
    assert all(a[1] + 1 == b[0] for a, b in zip(dc.PICK_GEOM, dc.PICK_GEOM[1:]))
    assert all(f[0] * f[1] >= top for _, top, dflt, off in dc.PICK_GEOM for f in (dflt, off))
    for name, (paired, reads, _) in dc.batches(gi).items():
        assert dc.longest(reads) == hi, name
        assert min(int(reads[1].min()), int(reads[3].min()) if paired else 999) >= 16, name
    if gi == dc.BIS_GEOM:
        for name in ("seam", "sweep"):
            assert dc.longest(dc.bisulfite_batch(name)[1]) == hi


@pytest.mark.parametrize("gi", GI, ids=IDS)
def test_seam_gaps_are_planted_at_every_seam_and_found(gi):
    lanes, W, hi = dc.GEOMS[gi]
    paired, reads, meta = dc.batches(gi)["seam"]
    # the plan: pads of 0 (16 x 19: 26), 1, W - 1, W, W + 1 and of several lanes; every seam with the gap before, at and behind it
    pads = sorted(set((lanes * W - meta["mm"]).tolist()))
    base = lanes * W - hi
    assert pads[:5] == [base, base + 1, base + W - 1, base + W, base + W + 1] and pads[5] >= 3 * W, pads
    full = meta[meta["mm"] == hi]
    assert set(zip(full["g"].tolist(), full["off"].tolist())) >= {(g, off) for g in range((base + W + 1) // W, lanes) for off in (-1, 0, 1)}
    assert set(meta["b"].tolist()) == set(dc.GAP_SIZES) and meta["ins"].any() and (~meta["ins"]).any()
    assert (meta["g"] * W - (lanes * W - meta["mm"]) + meta["off"] == meta["p"]).all()
    assert ((meta["p"] >= 1) & (meta["p"] <= meta["mm"] - 1)).all()
    assert len(meta) >= (1300 if lanes == 16 else 600), len(meta)
    # both strands and both reads carry gapped ends
    for k in ("first", "reverse"):
        assert 0.4 * len(meta) < int(meta[k].sum()) < 0.6 * len(meta), k
    r = _oracle(gi, "seam")
    mapped = _subject(r, meta["first"]) > 0
    want_del = int(meta["b"][~meta["ins"]].sum())
    n_ins = int(meta["ins"].sum())
    gapped = _gapped_alignments(reads, r)
    print(dc.geom_name(gi), "seam pairs", len(meta), "planted ends mapped", int(mapped.sum()), "deletion increments", r["dels"], "of", want_del,
          "insertions logged", r["n_ins"], "of", n_ins, "gapped alignments", gapped)
    assert mapped.all(), meta[~mapped]
    assert r["dels"] >= 0.95 * want_del
    assert r["n_ins"] >= 0.85 * n_ins
    # gapped alignments that run A walks in this geometry, counted on the seam batch alone
    assert gapped >= (1000 if lanes == 16 else 500)


@pytest.mark.parametrize("gi", GI, ids=IDS)
def test_sweep_maps_every_length(gi):
    lanes, W, hi = dc.GEOMS[gi]
    paired, reads, meta = dc.batches(gi)["sweep"]
    assert meta["mm"].tolist() == [mm for mm in range(16, hi + 1) for _ in range(4)] and meta["kind"].tolist() == [0, 1, 2, 3] * (hi - 15)
    subject = np.where(meta["first"], reads[1], reads[3])
    assert np.array_equal(subject, meta["mm"])
    r = _oracle(gi, "sweep")
    both = (r["m1"] > 0) & (r["m2"] > 0)
    by_kind = [float(both[meta["kind"] == k].mean()) for k in range(4)]
    short = (reads[1] < 32) | (reads[3] < 32)
    clipped = sum(int((d["win_len"][i, :d["n_hits"][i]] < reads[2 * w + 1][i] + 21).sum()) for w, d in enumerate(r["d"]) for i in np.nonzero(d["n_hits"])[0])
    print(dc.geom_name(gi), "sweep pairs", len(both), "both ends mapped %.3f" % both.mean(), "by kind", ["%.3f" % x for x in by_kind],
          "pairs with a read under 32 bases", int(short.sum()), "mapped %.3f" % both[short].mean(), "clipped windows", clipped)
    assert both.mean() >= 0.90
    assert by_kind[0] == by_kind[1] == by_kind[2] == 1.0
    assert short.sum() >= 100 and both[short].mean() >= 0.90
    assert clipped >= 20


@pytest.mark.parametrize("gi", GI, ids=IDS)
def test_twins_have_several_hits_and_odd_windows_hold_odd_letters(gi):
    r = _oracle(gi, "twins")
    nh = np.concatenate([d["n_hits"] for d in r["d"]])
    print(dc.geom_name(gi), "twins: ends with two or more hits %.3f" % (nh >= 2).mean(), "mapped ends", int((r["m1"] > 0).sum() + (r["m2"] > 0).sum()))
    assert (nh >= 2).mean() >= 0.35
    r = _oracle(gi, "odd")
    genome = dc.index()["genome"]
    plain = np.zeros(256, bool)
    plain[list(b"ACGT")] = True
    odd_windows = sum(int(not plain[genome[d["win_start"][i, k]:d["win_start"][i, k] + d["win_len"][i, k]]].all())
                      for d in r["d"] for i in np.nonzero(d["n_hits"])[0] for k in range(d["n_hits"][i]))
    mapped = int((r["m1"] > 0).sum() + (r["m2"] > 0).sum())
    print(dc.geom_name(gi), "odd: mapped ends", mapped, "of", 2 * len(r["m1"]), "windows with a letter outside ACGT", odd_windows,
          "deletion increments", r["dels"])
    assert mapped >= len(r["m1"])
    assert odd_windows >= 50


@pytest.mark.parametrize("gi", GI, ids=IDS)
def test_tiny_batches_are_the_first_gapped_ends_and_map(gi):
    lanes, W, hi = dc.GEOMS[gi]
    b = dc.batches(gi)
    sizes = dc.tiny_sizes(lanes)
    assert sizes == (1, 64 // lanes - 1, 64 // lanes, 64 // lanes + 1)
    paired, seam, meta = b["seam"]
    for n in sizes:
        paired, reads, m = b["tiny%d" % n]
        assert not paired and len(reads[1]) == n and (reads[1] == hi).all()
        for i in range(n):
            row, ln = dc.gapped_end(seam, meta, i)
            assert ln == hi and np.array_equal(reads[0][i], row)
        o = oracle_py.Oracle(dc.index(), paired=False, **dc.PARAMS)
        m1 = o.map_batch(*reads, threads=8)[0]
        assert (m1 > 0).all(), (n, m1)
