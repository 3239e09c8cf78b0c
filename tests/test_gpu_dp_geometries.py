"""The full DP (pm_sw_kernel, fp64 affine gaps) and the traceback that follows its direction nibbles (pm_walk_kernel) in each of the
six lane geometries pick_geom instantiates, on dp_cases.py's batches: gaps at every lane seam, every read length, ends with several
hits, odd reference letters, launches of fewer problems than a wave takes.  test_dp_cases_cpu.py holds the conditions on the inputs.

Run A maps them with PEMAP_GAPLESS=0 -- every problem through the full DP, every winner walked -- in ONE child process (the knobs are
read when the object is made) that goes through the geometries in ascending order on one object and then repeats the 8 x 13 seam
batch, so that the direction buffer, the path words and the dump slab it meets were sized by the widest geometry; the bisulfite seam
and sweep batches of 16 x 13 go through a second object of the same child.  Run B maps the same batches with the default knobs in
this process (8 x 19 does not exist there: its batches run at 16 x 10), where the full DP sees what the gapless rule, the band and its
gate leave.  Both are compared with the oracle, exactly: coordinates, classes, summary, pileup, insertions, per end the hit list and
windows, per hit the fp64 score bits and the start cell; run A also by run_stats that the full DP did all of it; both that
pemap_dev_sw_geom names the geometry the batch was made for."""
import functools
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import dp_cases as dc
import oracle_py

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DBG_KEYS = ("spot", "orient", "win_start", "win_len", "score", "start_k", "start_i")
REPEAT = "again"        # the 8 x 13 seam batch once more, after the widest geometry
BIS = "bis"             # the bisulfite object's batches


def _batch(tag, name):
    """tag: a geometry's number, REPEAT or BIS -> (paired, reads, meta, bisulfite, hi)"""
    if tag == BIS:
        return dc.bisulfite_batch(name) + (True, dc.GEOMS[dc.BIS_GEOM][2])
    gi = 0 if tag == REPEAT else tag
    return dc.batches(gi)[name] + (False, dc.GEOMS[gi][2])


def _plan():
    """the child's batches in its order: (tag, name)"""
    plan = [(gi, name) for gi in range(len(dc.GEOMS)) for name in dc.batches(gi)]
    return plan + [(REPEAT, "seam"), (BIS, "seam"), (BIS, "sweep")]


def _key(tag, name):
    return "%s.%s" % (tag if isinstance(tag, str) else dc.geom_name(tag), name)


@functools.lru_cache(maxsize=None)
def _expected(tag, name):
    """the oracle's results for one batch on an empty pileup (computed once, shared by both runs, never modified)"""
    if tag == REPEAT:
        return _expected(0, name)
    paired, reads, meta, bis, hi = _batch(tag, name)
    o = oracle_py.Oracle(dc.index(bis), paired=paired, bisulfite=bis, **dc.PARAMS)
    m1, m2, mt, d1, d2 = o.map_batch(*reads, debug=True, threads=8)
    ds = []
    for d in (d1, d2) if paired else (d1,):
        k = max(1, int(d["n_hits"].max()))
        ds.append(dict(n_hits=d["n_hits"].copy(), spot=d["spot"][:, :k].copy(), orient=d["orient"][:, :k].copy(),
                       win_start=d["win_start"][:, :k].astype(np.int64) & 0xFFFFFFFF, win_len=d["win_len"][:, :k].copy(),
                       score=d["score"][:, :k].copy(), start_k=d["start"][:, :k, 0].copy(), start_i=d["start"][:, :k, 1].copy()))
    return dict(m1=m1, m2=m2, mt=mt, d=ds, counts=o.counts().copy(), ins=o.insertions(), summary=np.array(o.summary()))


def _map_one(dev, tag, name):
    """one batch on the device, on an empty pileup -> its outputs as arrays (the hit records cut to the longest hit list)"""
    paired, reads, meta, bis, hi = _batch(tag, name)
    n = len(reads[1])
    dev.set_params(paired=paired, bisulfite=bis, **dc.PARAMS)
    dev.reset_pileup()
    m1, m2, mt = dev.map_batch(*reads)
    stats, _ = dev.run_stats()
    dbg = dev.debug_hits(2 * n if paired else n)
    counts, ins = dev.fetch_pileup()
    summary = dev.summary()
    k = max(1, int(dbg["n_hits"].max()))
    out = dict(m1=m1, m2=m2 if paired else np.zeros(0, np.uint32), mt=mt, counts=counts, summary=np.array(summary), n_hits=dbg["n_hits"],
               geom=np.array(dev.sw_geom(hi)), stats=np.frombuffer(json.dumps(stats).encode(), np.uint8),
               ins=np.frombuffer(json.dumps([[p, s.decode("latin1")] for p, s in ins]).encode(), np.uint8))
    for key in DBG_KEYS:
        out[key] = dbg[key][:, :k]
    return out


def _rows(meta, pairs):
    """the seam plan's rows of some pairs, for a failure's message: (mm, g, off, p, b, insertion, ...)"""
    if meta is None or "g" not in (meta.dtype.names or ()):
        return pairs[:10]
    return [tuple(meta[i]) for i in pairs[:10] if i < len(meta)]


def _compare(got, tag, name):
    paired, reads, meta, bis, hi = _batch(tag, name)
    exp = _expected(tag, name)
    t = _key(tag, name)
    step = 2 if paired else 1
    # the hit lists first: a wrong score names its end and, in a seam batch, its gap
    for which, od in enumerate(exp["d"]):
        nh = got["n_hits"][which::step]
        assert np.array_equal(nh, od["n_hits"]), (t, which, _rows(meta, np.nonzero(nh != od["n_hits"])[0]))
        k = od["score"].shape[1]
        assert got["score"].shape[1] >= k, (t, got["score"].shape, k)
        live = np.arange(k)[None, :] < nh[:, None]
        for key in DBG_KEYS:
            a, b = got[key][which::step, :k], od[key]
            if key == "score":
                a, b = np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64)
            same = (a == b) | ~live
            assert same.all(), (t, key, "read %d" % (which + 1), _rows(meta, np.nonzero(~same.all(axis=1))[0]))
    assert np.array_equal(got["m1"], exp["m1"]), (t, _rows(meta, np.nonzero(got["m1"] != exp["m1"])[0]))
    if paired:
        assert np.array_equal(got["m2"], exp["m2"]), (t, _rows(meta, np.nonzero(got["m2"] != exp["m2"])[0]))
    assert np.array_equal(got["mt"], exp["mt"]), t
    assert np.array_equal(got["summary"], exp["summary"]), (t, got["summary"], exp["summary"])
    assert np.array_equal(got["counts"], exp["counts"]), (t, np.nonzero((got["counts"] != exp["counts"]).any(axis=1))[0][:10])
    ins = sorted((p, s.encode("latin1")) for p, s in json.loads(got["ins"].tobytes().decode()))
    assert ins == exp["ins"], (t, len(ins), len(exp["ins"]))
    return exp


def _check_full_dp(st, got, exp, t, twins):
    """run A: the gapless rule, the band and its gate took nothing, every winner was walked, and the DP's cell counts are the windows'"""
    mapped = int((got["m1"] > 0).sum() + (got["m2"] > 0).sum())
    hits = single = multi = 0
    for d in exp["d"]:
        nh = d["n_hits"]
        live = np.arange(d["win_len"].shape[1])[None, :] < nh[:, None]
        cells = np.where(live, np.maximum(d["win_len"], 0).astype(np.int64) * d["mm"][:, None], 0).sum(axis=1)
        hits += int(nh.sum())
        single += int(cells[nh == 1].sum())
        multi += int(cells[nh >= 2].sum())
    print(t, "mapped ends", mapped, "hits", hits, {k: st[k] for k in ("sw_score", "sw_dirs", "cells_score", "cells_dirs", "walks", "walked", "redo", "n_ins")})
    assert st["gapless"] == 0 and st["banded"] == 0 and st["gated"] == 0, (t, st)
    assert st["walked"] == st["walks"] == mapped, (t, st, mapped)
    assert st["sw_score"] == hits, (t, st, hits)
    assert st["cells_score"] == multi, (t, st, multi)
    assert st["cells_dirs"] >= single and (st["redo"] > 0 or st["cells_dirs"] == single), (t, st, single)
    if twins:
        assert st["redo"] > 0 and st["cells_score"] > 0, (t, st)


def _with_lengths(tag, name):
    """the expected hit records with each end's read length beside them (the cell counts need it)"""
    paired, reads, meta, bis, hi = _batch(tag, name)
    exp = _expected(tag, name)
    return dict(exp, d=[dict(d, mm=reads[2 * w + 1].astype(np.int64)) for w, d in enumerate(exp["d"])])


# ---- run A: the child
def _worker(out_path):
    """maps every batch of _plan() with whatever knobs the environment sets and saves the outputs; a HIP error ends it there"""
    sys.path.insert(0, ROOT)
    from pecaller_amd import PemapDev
    out = {}
    devs = {}
    t0 = time.time()
    for tag, name in _plan():
        bis = tag == BIS
        if bis not in devs:
            ix = dc.index(bis)
            devs[bis] = PemapDev(0)
            devs[bis].build_index(ix["genome"], ix["contig_len"], bisulfite=bis)
            print("object with its index, bisulfite %d: %.1f s" % (bis, time.time() - t0), flush=True)
        print("%.2f s: %s" % (time.time() - t0, _key(tag, name)), flush=True)
        for k, v in _map_one(devs[bis], tag, name).items():
            out[_key(tag, name) + "." + k] = v
    for d in devs.values():
        d.close()
    print("mapped in %.1f s" % (time.time() - t0), flush=True)
    np.savez(out_path, **out)


# One child for all six geometries.  Its time is the making of its two objects (1.2 s and about 3 s: the second finds no room for the
# look-up replicas beside the first); the 51 batches map in 0.3 s.  Two children, one for the geometries of 8 lanes and one for those
# of 16, took 1.8 s and 12.7 s: a process that allocates right after another one has freed 190 GB waits for that.
@pytest.fixture(scope="module")
def run_a(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("dp_geometries") / "full_dp.npz")
    t0 = time.time()
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=dict(os.environ, PEMAP_GAPLESS="0"), cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    print("child: %.1f s\n%s" % (time.time() - t0, r.stdout.decode()[-4000:]))
    assert r.returncode == 0, r.stdout.decode()[-2000:]
    return np.load(out)


def _from_child(z, tag, name):
    pre = _key(tag, name) + "."
    return {k[len(pre):]: z[k] for k in z.files if k.startswith(pre)}


# ---- run B: this process, default knobs
@pytest.fixture(scope="module")
def run_b():
    from pecaller_amd import PemapDev
    devs = {}

    def dev_for(bis):
        if bis not in devs:
            ix = dc.index(bis)
            devs[bis] = PemapDev(0)
            devs[bis].build_index(ix["genome"], ix["contig_len"], bisulfite=bis)
        return devs[bis]
    yield dev_for
    for d in devs.values():
        d.close()


CASES = [(gi, kind) for gi in range(len(dc.GEOMS)) for kind in dc.KINDS] + [(BIS, "seam"), (BIS, "sweep")]


def _case_id(c):
    return "%s-%s" % (c[0] if isinstance(c[0], str) else dc.geom_name(c[0]), c[1])


def _names(tag, kind):
    return dc.names_of(tag, kind) if not isinstance(tag, str) else [kind]


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_full_dp_everywhere(case, run_a):
    tag, kind = case
    gi = dc.BIS_GEOM if tag == BIS else tag
    for name in _names(tag, kind):
        got = _from_child(run_a, tag, name)
        assert tuple(got["geom"]) == dc.GEOMS[gi][:2] == dc.picked(dc.GEOMS[gi][2], gapless_on=False), (_key(tag, name), got["geom"])
        _compare(got, tag, name)
        _check_full_dp(json.loads(got["stats"].tobytes().decode()), got, _with_lengths(tag, name), _key(tag, name), kind == "twins")


def test_full_dp_8x13_again_in_buffers_sized_for_the_widest(run_a):
    got = _from_child(run_a, REPEAT, "seam")
    first = _from_child(run_a, 0, "seam")
    assert tuple(got["geom"]) == (8, 13)
    assert sorted(got) == sorted(first)
    for k in got:
        if k != "stats":
            assert np.array_equal(got[k], first[k]), k
    _compare(got, REPEAT, "seam")
    _check_full_dp(json.loads(got["stats"].tobytes().decode()), got, _with_lengths(REPEAT, "seam"), _key(REPEAT, "seam"), False)


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_default_route(case, run_b):
    tag, kind = case
    gi = dc.BIS_GEOM if tag == BIS else tag
    dev = run_b(tag == BIS)
    for name in _names(tag, kind):
        got = _map_one(dev, tag, name)
        assert tuple(got["geom"]) == dc.picked(dc.GEOMS[gi][2]), (_key(tag, name), got["geom"])
        _compare(got, tag, name)
        st = json.loads(got["stats"].tobytes().decode())
        print(_key(tag, name), {k: st[k] for k in ("gapless", "banded", "gated", "sw_score", "sw_dirs", "walks", "walked", "redo")})
        assert st["walks"] == int((got["m1"] > 0).sum() + (got["m2"] > 0).sum()) and st["walked"] <= st["walks"], (_key(tag, name), st)


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    _worker(sys.argv[1])
