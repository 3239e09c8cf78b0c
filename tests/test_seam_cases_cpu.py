"""What the plans of tests/seam_cases.py must fulfil before tests/test_gpu_chunk_seam.py runs them on the device: the chunk arithmetic
that takes run_slice down each of its paths (written out here from the two constants, not read from the library), the read lengths
that move the kernels' geometry, and -- from the oracle -- that every ragged batch maps, walks gapped alignments and, for the plan
`params`, tells the two distance limits apart.

Oracle time: the ragged_reads batches of all plans (16 x 200 + 2,400 + 900 pairs, the first `params` batch three times) take the oracle
0.9 s on 8 threads, 1.4 s with the making of the reads; the whole module runs in about 3 s."""
import hashlib
import numpy as np
import pytest
import seam_cases as sc

CHUNK, TABLE = 64, 256            # PEMAP_CHUNK_PAIRS of the child processes, PM_MAX_CHUNKS


def nch(n):
    return (n + CHUNK - 1) // CHUNK


def test_constants_are_the_ones_the_plans_were_made_for():
    assert (sc.CHUNK, sc.MAX_CHUNKS, sc.STRIDE, sc.N_R150) == (CHUNK, TABLE, 304, 20000)


def test_uneven_covers_the_set_and_fills_the_table_more_than_once():
    cuts = sc.uneven()
    assert cuts[0][0] == 0 and cuts[-1][1] == 20000 and all(a[1] == b[0] for a, b in zip(cuts[:-1], cuts[1:]))
    sizes = [b - a for a, b in cuts]
    assert sizes[0] == 1000 == 15 * CHUNK + 40 and max(sizes) == 1000       # 15 full chunks and a tail; the ring's capacity (1,024) holds every batch
    assert {1, 63, 64, 65, 127, 128, 129, 1000} <= set(sizes)
    assert sum(nch(n) for n in sizes) > TABLE
    # the table fills in the middle of a batch sequence: some batch finds fewer free entries than it has chunks
    at, absorbs = 0, 0
    for n in sizes:
        if at + nch(n) > TABLE:
            at, absorbs = 0, absorbs + 1
        at += nch(n)
    assert absorbs >= 1


def test_exact_fill_stands_at_the_table_size_after_batch_64():
    cuts = sc.exact_fill()
    assert len(cuts) == 70 and cuts[-1][1] == 17920 and all(b - a == 256 and nch(b - a) == 4 for a, b in cuts)
    assert sum(nch(b - a) for a, b in cuts[:64]) == TABLE                   # run_chunks + nch == 256: continues
    assert sum(nch(b - a) for a, b in cuts[:65]) == TABLE + 4               # the 65th does not fit
    # continued runs: 63 behind the first, 5 behind the 65th
    assert 63 + (70 - 65) == 68


def test_one_run_has_its_chunk_raised():
    (a, b), = sc.one_run()
    n = b - a
    assert n == 20000 and nch(n) == 313 > TABLE
    chunk = (n + TABLE - 1) // TABLE
    assert chunk == 79 and (n + chunk - 1) // chunk == 254
    assert sc.chunks_of(n) == (254, 79) and sc.chunks_of(1000) == (16, 64) and sc.chunks_of(1) == (1, 1)


def test_lengths_visit_every_template_and_geometry_on_both_sides_of_each_edge():
    plan = sc.lengths()
    his = [b["hi"] for b in plan]
    assert his == [60, 104, 105, 112, 113, 160, 161, 208, 209, 256, 257, 278, 150, 40, 278, 100]
    for b in plan:
        b1, l1, b2, l2 = b["reads"]
        assert len(l1) == len(l2) == 200 and b1.shape == b2.shape == (200, 304)
        assert l1[0] == b["hi"] == max(l1.max(), l2.max()), b["hi"]         # the bound is attained, by the forced first end at least
        assert min(l1.min(), l2.min()) >= max(16, b["lo"] - 3) and b["lo"]      # (- 3: ragged_reads' planted deletion shortens an end) == (b["hi"] if b["hi"] in (104, 257) else 16)
        assert set(np.unique(b1[0, :l1[0]])) <= set(b"ACGT")
    assert {sc.seg_template(h) for h in his} == {7, 10, 13, 16, 19}
    assert {sc.sw_geom(h) for h in his} == {(8, 13), (16, 10), (16, 13), (16, 16), (16, 19)}
    for e in sc.SEG_EDGES:
        assert e in his and e + 1 in his and sc.seg_template(e) != sc.seg_template(e + 1)
    for e in sc.GEOM_EDGES:
        assert e in his and e + 1 in his and sc.sw_geom(e) != sc.sw_geom(e + 1)
    # the bound that never shrinks: 11 strict new maxima behind the first batch, then four batches below it
    bound, rises, below = his[0], 0, []
    for k, h in enumerate(his[1:], 1):
        if h > bound:
            bound, rises = h, rises + 1
        else:
            below.append(k)
    assert rises == 11 and below == [12, 13, 14, 15] and bound == 278


def test_remade_changes_stride_capacity_and_bound():
    plan = sc.remade()
    assert [(len(b["reads"][1]), b["stride"], b["reads"][0].shape[1]) for b in plan] == [(300, 304, 304), (300, 160, 160), (1500, 160, 160), (300, 304, 304)]
    mx = [int(max(b["reads"][1].max(), b["reads"][3].max())) for b in plan]
    assert mx[0] > 256 and mx[1] <= 150 and mx[2] <= 120 and mx[3] > 256    # 16 x 19, down to at most 120 behind the re-set-up, up again
    assert 1500 > 1024 >= 300                                               # the third batch exceeds the ring's capacity
    assert all(b["reads"][0].flags["C_CONTIGUOUS"] and b["reads"][2].flags["C_CONTIGUOUS"] for b in plan)


def test_ragged_reads_draws_what_it_drew_in_test_gpu_edge():
    """the function moved here from tests/test_gpu_edge.py: same seed, same reads"""
    b1, l1, b2, l2 = sc.ragged_reads(1294, 60, 16, 278)
    h = hashlib.md5(b1.tobytes() + l1.tobytes() + b2.tobytes() + l2.tobytes()).hexdigest()
    assert h == RAGGED_MD5, h


RAGGED_MD5 = "d3a919e0932ef8fa5c49843428a928ec"        # of the function as it stood in tests/test_gpu_edge.py


@pytest.mark.parametrize("plan", ["lengths", "remade", "params"])
def test_every_ragged_batch_maps_and_walks_a_gap(plan):
    per = sc.oracle(plan)["per"]
    prev = (0, 0)
    for k, p in enumerate(per):
        n = len(p["m1"])
        mapped = (p["m1"] > 0) | ((p["m2"] > 0) if p["m2"] is not None else False)
        assert 2 * int(mapped.sum()) >= n, (plan, k, int(mapped.sum()))
        if plan == "params" and k == 2:
            prev = (0, 0)                # (the single-end batch has an oracle of its own)
        assert p["n_ins"] - prev[0] >= 1 or p["n_del"] - prev[1] >= 1, (plan, k)
        prev = (p["n_ins"], p["n_del"])


def test_params_batches_tell_the_two_distance_limits_apart():
    bs = sc.params()
    per = sc.oracle("params")["per"]
    lo, hi = 4 * sc.PARAMS_MAX_DIST[1], 4 * sc.PARAMS_MAX_DIST[0]
    assert (lo, hi) == (400, 2000)
    for b, p in zip(bs[:2], per[:2]):
        both = (p["m1"] > 0) & (p["m2"] > 0)
        d = (p["m1"].astype(np.int64) - p["m2"].astype(np.int64)) % (1 << 32)
        assert int((both & (d >= lo) & (d < hi)).sum()) >= 1
        # the fold of the delivered batch (restated in seam_cases.fold) under the limit it was submitted with and under the later one
        _, l1, _, l2 = b["reads"]
        wide, narrow = (sc.fold(p["m1"], p["m2"], p["mt"], l1, l2, True, m) for m in sc.PARAMS_MAX_DIST)
        assert wide[2] != narrow[2] and wide[3] != narrow[3] and np.array_equal(wide[[0, 1]], narrow[[0, 1]]) and np.array_equal(wide[4:], narrow[4:])
        # and folded as single-end (what a delivery behind set_params (paired = 0) made of it): [0] and [1] lose the second ends
        single = sc.fold(p["m1"], None, p["mt"], l1, l2, False, sc.PARAMS_MAX_DIST[1])
        assert single[0] < wide[0] and single[1] < wide[1] and single[3] == 0
    # the restated fold is the oracle's: the first batch alone, under either limit (the limit also moves classes: mapped afresh)
    o = sc.oracle("params_dist")
    _, l1, _, l2 = bs[0]["reads"]
    p = o["per"][0]
    assert np.array_equal(sc.fold(p["m1"], p["m2"], p["mt"], l1, l2, True, 500), o["final"]["summary"])
    assert o["final"]["summary"][2] != o["final"]["summary_narrow"][2] and o["final"]["summary"][3] != o["final"]["summary_narrow"][3]
    # the plan's sum: two paired batches under 500 and the single-end batch under 100
    tot = sum(sc.fold(q["m1"], q["m2"], q["mt"], b["reads"][1], b["reads"][3], b["paired"], b["max_dist"]) for b, q in zip(bs, per))
    assert np.array_equal(tot, sc.oracle("params")["final"]["summary"])

