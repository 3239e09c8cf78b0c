"""The pair / single-end selection on the inputs of pair_cases.py, CPU only: the plain-Python restatement (pair_cases.select_py)
against the oracle for every parameter set, and floors that say the inputs reach what they were built for -- every mapping class
the reference assigns, both distance limits, the score threshold, the second end's tie count read at the first end's index, the
-1.0 fill, long hit lists.  The floors are checked on the oracle's results alone; they measure nothing, they make the inputs worth
running (tests/test_gpu_pair_select.py maps the same inputs on the device, test_oracle_golden.py ties the oracle to the reference
on them).

Reads changed by each deliberate error of select_py, per parameter set, as measured (the floor below asks for 5 somewhere):

  set           best2  max_lt  min_gt  no_orient  no_slip  good_gt  clamp
  baseline        135       8      12        191      171        0      8
  narrow          171      43      44         87        1        0      8
  on_score        109      37      38         18        0      311      6
  above_score      97      37      38         13        0      206      6
  empty           197       0       0          0        0        0      8
  zero            197      12      12          0        0        0      8
  wide             55       9      12        191      452        0      3
  on_score150     111      37      38         24        0      462      0
  single_on         0       0       0          0        0      188      0
  single_above      0       0       0          0        0      123      0
"""
import numpy as np
import pytest

import pair_cases as pc


def _oracle_rows(name):
    e = pc.expected(name)
    m2 = e["m2"] if e["m2"] is not None else np.zeros_like(e["m1"])
    return np.stack([e["mt"].astype(np.int64), e["m1"].astype(np.int64), m2.astype(np.int64)], axis=1)


def test_genome_and_reads_are_what_the_generator_says():
    g = pc.genome()
    assert len(g["contigs"]) == pc.NC and all(len(c) == pc.CL for c in g["contigs"])
    assert len(g["family"]) >= 24
    cs = g["contigs"]
    for c, s, d in g["near"]:
        assert np.array_equal(cs[c][s:s + pc.NEAR], cs[c][s + d:s + d + pc.NEAR]) and 140 <= d <= 400
    # unequal copies: the places of a block with several copies do not all lie equally far from the source
    uneven = 0
    for places in g["blocks"]:
        c0, s0 = places[0]
        far = [int((cs[c][s:s + pc.BLOCK] != cs[c0][s0:s0 + pc.BLOCK]).sum()) for c, s in places[1:]]
        uneven += len(set(far)) > 1
    assert uneven >= 5
    b1, l1, b2, l2 = pc.reads(100)
    assert len(l1) == pc.PAIRS and (l1 == 100).all() and (l2 == 100).all()
    assert (pc.reads(150)[1] == 150).all()


def test_threshold_sits_on_a_score():
    """`score >= len * min_align * 1.0` decides only where the product IS a score: the on_score sets hit one exactly, the
    above_score sets are the next double for which the product exceeds it"""
    for L in (100, 150):
        score, on, above = pc.score_on_threshold(L)
        assert L * on * 1.0 == score and L * above * 1.0 > score and above == np.nextafter(on, 1.0)
        hit = sum(int((d["score"] == score).sum()) for d in pc.expected("narrow" if L == 100 else "on_score150")["d"])
        assert hit >= 100, (L, score, hit)
    assert pc.score_on_threshold(100)[:2] == (96.0, 0.96)           # three mismatches in 100 bases: 97 - 3 / 3


@pytest.mark.parametrize("name", pc.SETS)
def test_restatement_equals_oracle(name):
    got = pc.restated(name)
    exp = _oracle_rows(name)
    bad = np.nonzero((got != exp).any(axis=1))[0]
    assert len(bad) == 0, (name, len(bad), bad[:10], got[bad[:3]].tolist(), exp[bad[:3]].tolist())


def test_every_class_is_reached():
    total = np.zeros(9, np.int64)
    for name in pc.PAIRED_SETS:
        total += np.bincount(pc.expected(name)["mt"], minlength=9)
    print("reads per class over the paired sets", total.tolist())
    for cls in (0, 1, 2, 3, 4, 5, 7, 8):
        assert total[cls] >= 5, (cls, total.tolist())
    assert total[pc.FRAG_MIS] == 0          # never assigned by the reference
    # unpaired runs know three outcomes
    single = np.bincount(pc.expected("single_on")["mt"], minlength=9)
    assert all(single[c] >= 5 for c in (pc.UNIQUE_SINGLE, pc.NON_NO, pc.NEITHER_MAP)) and single.sum() == single[[2, 7, 8]].sum()
    # an empty distance range leaves no proper pair, degenerate limits leave a few
    assert np.bincount(pc.expected("empty")["mt"], minlength=9)[[0, 1, 4]].sum() == 0
    assert np.bincount(pc.expected("zero")["mt"], minlength=9)[0] >= 5


@pytest.mark.parametrize("variant", pc.VARIANTS)
def test_every_variant_is_caught(variant):
    """each deliberate error changes at least 5 reads in some set: select_py with it would fail test_restatement_equals_oracle"""
    changed = {name: int((pc.restated(name, variant) != pc.restated(name)).any(axis=1).sum()) for name in pc.SETS}
    print(variant, changed)
    assert max(changed.values()) >= 5, (variant, changed)
    if variant == "min_gt":
        assert changed["narrow"] >= 5           # (needs a min_dist that fragments can fall on)
    if variant == "good_gt":
        assert changed["baseline"] == 0 and changed["on_score"] >= 5 and changed["single_on"] >= 5


def test_threshold_sets_differ():
    for a, b in (("on_score", "above_score"), ("single_on", "single_above")):
        n = int((pc.expected(a)["mt"] != pc.expected(b)["mt"]).sum())
        print(a, b, "classes that differ", n)
        assert n >= 5, (a, b, n)


def test_long_hit_lists_and_limit_distances():
    d1, d2 = pc.expected("narrow")["d"]
    n1, n2 = d1["n_hits"].astype(np.int64), d2["n_hits"].astype(np.int64)
    assert int((n1 * n2 >= 400).sum()) >= 5
    # pairs of two single-hit ends on opposite strands whose spot distance sits one below, on, on and one above the limits
    one = (n1 == 1) & (n2 == 1) & (d1["orient"][:, 0] != d2["orient"][:, 0])
    dist = np.abs(d1["spot"][:, 0].astype(np.int64) - d2["spot"][:, 0].astype(np.int64))
    lo, hi = pc.NARROW
    for x in (lo - 1, lo, hi, hi + 1, 0, 500, 501, 5000, 5001):
        n = int((one & (dist == x)).sum())
        print("pairs at spot distance", x, ":", n)
        assert n >= 5, (x, n)
    # ... and the limits decide them: inside is a unique pair, outside a unique mis-size
    mt = pc.expected("narrow")["mt"]
    for x, cls in ((lo - 1, pc.UNIQUE_MIS), (lo, pc.UNIQUE_MATE), (hi, pc.UNIQUE_MATE), (hi + 1, pc.UNIQUE_MIS)):
        assert (mt[one & (dist == x)] == cls).all(), x


def test_the_fill_is_read():
    """no proper pair, the first end's best hit at an index past the end of the second end's list of three or more: the -1.0 fill
    is what the second end's ties are measured against"""
    d1, d2 = pc.expected("empty")["d"]
    n = 0
    for i in np.nonzero((d1["n_hits"] > 3) & (d2["n_hits"] >= 3))[0]:
        n += int(np.argmax(d1["score"][i, :d1["n_hits"][i]])) >= d2["n_hits"][i]
    assert n >= 5, n
