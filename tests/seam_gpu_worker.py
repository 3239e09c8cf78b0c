"""Runs the plans of tests/seam_cases.py on a PemapDev and checks them: the r150 plans against the reference's golden outputs, the ragged
plans against the oracle, and pemap_dev_pipeline_stats for the path each submit took.  Imported by tests/test_gpu_chunk_seam.py, and run
as a child process by it (`main`), one per setting of the knobs that are read when an object is made.  Every GPU step is a plain call;
nothing is retried."""
import sys
import numpy as np
import fixtures
import seam_cases as sc

RUNS, CONT, TABLE, GEOM, CAP, SETUPS, NCH, K0 = range(8)      # pemap_dev_pipeline_stats


def make_dev():
    from pecaller_amd import PemapDev
    dev = PemapDev(0)
    ix = fixtures.index()
    dev.build_index(ix["genome"], ix["contig_len"])
    dev.set_params(paired=True, **sc.PARAMS)
    return dev


def leave_ring(dev):
    """The longest read the ring has seen lasts as long as the ring.  Staging a resident read set ends the ring (and accounts the pending
    run): the next submit sets it up again and the bound starts from nothing."""
    r1, l1, r2, l2 = fixtures.reads("r150")
    dev.stage_reads(r1[:16], l1[:16], r2[:16], l2[:16])


def begin(dev):
    """nothing pending, empty pileup -> the counters before the plan"""
    dev.sync()
    dev.reset_pileup()
    return dev.pipeline_stats()


def submit_all(dev, batches):
    """every batch submitted without a wait (a submit that finds the ring full delivers the oldest) -> tickets, the counters after each submit"""
    tickets, trace = [], []
    for rd in batches:
        tickets.append(dev.submit_batch(*rd))
        trace.append(dev.pipeline_stats())
    return tickets, trace


def check_began(s0, trace):
    """runs that did not begin a pipeline continued one; a pipeline begins with the plan's first run and behind every absorb"""
    d = [a - b for a, b in zip(trace[-1], s0)]
    began = sum(1 for t in trace if t[K0] == 0)
    assert d[RUNS] == len(trace) and d[CONT] == len(trace) - began, (d, began)
    assert began == 1 + d[TABLE] + d[GEOM] + d[CAP], (d, began)
    return d[:NCH]


# ---- the r150 plans
def run_r150(dev, cuts):
    r1, l1, r2, l2 = fixtures.reads("r150")
    s0 = begin(dev)
    tickets, trace = submit_all(dev, [(r1[a:b], l1[a:b], r2[a:b], l2[a:b]) for a, b in cuts])
    n = cuts[-1][1]
    m1, m2, mt = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.int32)
    for (a, b), t in reversed(list(zip(cuts, tickets))):
        m1[a:b], m2[a:b], mt[a:b] = dev.wait_batch(t)
    assert np.array_equal(m1, fixtures.golden_m("r150", 1)[:n]), np.nonzero(m1 != fixtures.golden_m("r150", 1)[:n])[0][:10]
    assert np.array_equal(m2, fixtures.golden_m("r150", 2)[:n]), np.nonzero(m2 != fixtures.golden_m("r150", 2)[:n])[0][:10]
    return s0, trace


def check_r150_totals(dev):
    """pileup, insertions and summary of the whole golden set, as test_batches_in_flight_equal_one_call checks them"""
    counts, ins = dev.fetch_pileup()
    fixtures.check_pileup_against_golden("r150", counts)
    names, contigs = fixtures.genome()
    assert fixtures.ins_to_named(ins, names, contigs) == fixtures.golden_insertions("r150")[0]
    tot, head, rows = fixtures.golden_summary("r150")
    sm = dev.summary()
    assert sm[0] == tot and rows["Unique Mate-Paired"] == sm[4] and rows["Neither Map"] == sm[12]
    assert head[3] == "%g" % (sm[1] / sm[0]) and head[7] == "%g" % (sm[2] / sm[3])


def plan_uneven(dev, continues=True):
    cuts = sc.uneven()
    s0, trace = run_r150(dev, cuts)
    check_r150_totals(dev)
    d = check_began(s0, trace)
    # (the plan is an object's first: its first batch, the largest, sets the ring up; no later one does)
    assert s0[SETUPS] == 0 and trace[0][SETUPS] == 1 and trace[-1][SETUPS] == 1, (s0, trace[0], trace[-1])
    if continues:
        assert d[TABLE] >= 1 and d[GEOM] == 0 and d[CAP] == 0, d
        assert all(t[NCH] == sc.chunks_of(b - a)[0] for t, (a, b) in zip(trace, cuts))
        assert any(t[K0] > 0 and t[NCH] > 1 for t in trace)                 # a continued run of several chunks
    else:                                                                    # PEMAP_PIPELINE=2: every run waits for the one before
        assert d[CONT] == 0 and d[CAP] == len(cuts) - 1 and d[TABLE] == 0 and d[GEOM] == 0, d
    return d


def plan_exact_fill(dev):
    cuts = sc.exact_fill()
    s0, trace = run_r150(dev, cuts)
    after = lambda k, i: trace[k - 1][i] - s0[i]                             # noqa: E731  (after submit k, counted from 1)
    assert after(64, CONT) == 63 and after(64, TABLE) == 0 and trace[63][K0] == 252 and trace[63][NCH] == 4, trace[63]
    assert after(65, TABLE) == 1 and trace[64][K0] == 0 and after(65, CONT) == 63, trace[64]
    assert after(70, CONT) == 68 and after(70, TABLE) == 1 and trace[69][K0] == 20, trace[69]
    d = check_began(s0, trace)
    # (the rest of the golden set, behind the plan, so that the pileup can be held against the reference's)
    r1, l1, r2, l2 = fixtures.reads("r150")
    a = cuts[-1][1]
    m1, m2, _ = dev.map_batch(r1[a:], l1[a:], r2[a:], l2[a:])
    assert np.array_equal(m1, fixtures.golden_m("r150", 1)[a:]) and np.array_equal(m2, fixtures.golden_m("r150", 2)[a:])
    check_r150_totals(dev)
    return d


def plan_one_run(dev):
    r1, l1, r2, l2 = fixtures.reads("r150")
    begin(dev)
    m1, m2, _ = dev.map_batch(r1, l1, r2, l2)
    st = dev.pipeline_stats()
    assert st[NCH] == 254 and st[K0] == 0, st
    assert dev.run_stats()[0]["chunks"] == 254
    assert np.array_equal(m1, fixtures.golden_m("r150", 1)) and np.array_equal(m2, fixtures.golden_m("r150", 2))
    check_r150_totals(dev)
    return st


# ---- the ragged plans
def check_batch(got, exp, what):
    m1, m2, mt = got
    assert np.array_equal(m1, exp["m1"]), (what, "m1", np.nonzero(m1 != exp["m1"])[0][:10])
    if exp["m2"] is not None:
        assert np.array_equal(m2, exp["m2"]), (what, "m2", np.nonzero(m2 != exp["m2"])[0][:10], int((m2 != 0).sum()))
    assert np.array_equal(mt, exp["mt"]), (what, "mapping_type")


def check_final(dev, fin, what):
    counts, ins = dev.fetch_pileup()
    assert np.array_equal(counts, fin["counts"]), (what, "pileup", np.nonzero((counts != fin["counts"]).any(axis=1))[0][:10])
    assert sorted(ins) == fin["ins"], (what, "insertions")
    assert np.array_equal(np.array(dev.summary()), fin["summary"]), (what, "summary", list(dev.summary()), list(fin["summary"]))


def plan_lengths(dev, one_chunk):
    plan, exp = sc.lengths(), sc.oracle("lengths")
    leave_ring(dev)
    s0 = begin(dev)
    tickets, trace = submit_all(dev, [b["reads"] for b in plan])
    res = [dev.wait_batch(t) for t in reversed(tickets)][::-1]
    for k, (got, e) in enumerate(zip(res, exp["per"])):
        check_batch(got, e, ("lengths", k, plan[k]["hi"]))
    check_final(dev, exp["final"], "lengths")
    d = check_began(s0, trace)
    assert d[GEOM] == 11 and d[TABLE] == 0 and d[CAP] == 0 and d[SETUPS] == 1, d
    bound = 0
    for k, (b, t) in enumerate(zip(plan, trace)):
        rose, bound = b["hi"] > bound, max(bound, b["hi"])
        prev = trace[k - 1] if k else s0
        assert t[NCH] == (1 if one_chunk else sc.chunks_of(sc.LENGTHS_PAIRS)[0]), (k, t)
        assert (t[GEOM] - prev[GEOM] == 1) == (rose and k > 0), (k, t, prev)        # a longer read absorbs the pipeline, and only that
        assert (t[K0] > 0 and t[CONT] - prev[CONT] == 1) == (not rose), (k, t, prev)   # a shorter or equal one continues under the bound
        assert dev.sw_geom(bound) == sc.sw_geom(bound)
    assert bound == 278 and all(trace[k][GEOM] == trace[11][GEOM] for k in (12, 13, 14, 15))    # 16 x 19 from the first 278 on
    return d


def plan_remade(dev):
    plan, exp = sc.remade(), sc.oracle("remade")
    leave_ring(dev)
    s0 = begin(dev)
    tickets, trace = [], []
    for k, b in enumerate(plan):
        tickets.append(dev.submit_batch(*b["reads"]))
        trace.append(dev.pipeline_stats())
        # every one of these submits re-makes the ring (the first one, another stride, a batch beyond the capacity, the stride again),
        # which delivers what is in flight: the earlier batches' result arrays hold their values when the submit returns
        assert trace[k][SETUPS] - s0[SETUPS] == k + 1, (k, trace[k])
        for j in range(k):
            check_batch(dev._inflight[tickets[j]][:3], exp["per"][j], ("remade", "behind submit", k, "batch", j))
    assert trace[2][SETUPS] - s0[SETUPS] == 3                        # first set-up, stride 160, capacity; the fourth is the stride of its rows
    for k, t in enumerate(tickets):                                  # the later wait returns 0 and changes nothing
        check_batch(dev.wait_batch(t), exp["per"][k], ("remade", "waited", k))
    check_final(dev, exp["final"], "remade")
    assert all(t[K0] == 0 for t in trace), trace                     # a re-made ring has accounted the pending run: nothing continues
    return [a - b for a, b in zip(trace[-1], s0)][:NCH]


def plan_params(dev):
    """set_params between batches in flight: they are delivered and folded under the values they were submitted with"""
    plan, exp = sc.params(), sc.oracle("params")
    dev.set_params(paired=True, **sc.PARAMS)
    begin(dev)
    t = [dev.submit_batch(*b["reads"]) for b in plan[:2]]
    dev.set_params(paired=False, **dict(sc.PARAMS, max_dist=sc.PARAMS_MAX_DIST[1]))
    t.append(dev.submit_batch(*plan[2]["reads"]))
    for k, tk in enumerate(t):
        check_batch(dev.wait_batch(tk), exp["per"][k], ("params", k))
    check_final(dev, exp["final"], "params")
    dev.set_params(paired=True, **sc.PARAMS)


def plan_params_dist(dev):
    """only max_dist changes, between the submit and the wait of one paired batch"""
    plan, exp = sc.params(), sc.oracle("params_dist")
    dev.set_params(paired=True, **sc.PARAMS)
    begin(dev)
    t = dev.submit_batch(*plan[0]["reads"])
    dev.set_params(paired=True, **dict(sc.PARAMS, max_dist=sc.PARAMS_MAX_DIST[1]))
    check_batch(dev.wait_batch(t), exp["per"][0], "params_dist")
    assert not np.array_equal(exp["final"]["summary"], exp["final"]["summary_narrow"])
    check_final(dev, exp["final"], "params_dist")
    dev.set_params(paired=True, **sc.PARAMS)


def plan_reset_refused(dev):
    """reset_pileup with a batch not waited for is refused and changes nothing"""
    from pecaller_amd import PemapError
    plan, exp = sc.params(), sc.oracle("params_dist")
    dev.set_params(paired=True, **sc.PARAMS)
    begin(dev)
    t = dev.submit_batch(*plan[0]["reads"])
    try:
        dev.reset_pileup()
        refused = ""
    except PemapError as e:
        refused = str(e)
    assert "not waited for" in refused, refused
    check_batch(dev.wait_batch(t), exp["per"][0], "reset_refused")
    check_final(dev, exp["final"], "reset_refused")
    dev.reset_pileup()                                               # delivered: allowed again
    assert not dev.summary().any() and dev.fetch_pileup()[1] == []


def main(which):
    dev = make_dev()
    out = {}
    if which == "A":          # PEMAP_CHUNK_PAIRS=64
        out["uneven"] = plan_uneven(dev)
        out["exact_fill"] = plan_exact_fill(dev)
        out["one_run"] = plan_one_run(dev)
        out["lengths"] = plan_lengths(dev, one_chunk=False)
    elif which == "B":        # PEMAP_CHUNK_PAIRS=64 PEMAP_REPLICAS=0: the reference's table layout, lists in HBM, vote and emit on the ALU stream
        assert dev.lookup_replicas()[0] == 0
        out["uneven"] = plan_uneven(dev)
        out["lengths"] = plan_lengths(dev, one_chunk=False)
    elif which == "C":        # PEMAP_CHUNK_PAIRS=64 PEMAP_PIPELINE=2: one stream, nothing continues
        out["uneven"] = plan_uneven(dev, continues=False)
    else:
        raise SystemExit("unknown child " + which)
    dev.close()
    print("counters", which, out)
    print("seam ok", which)


if __name__ == "__main__":
    main(sys.argv[1])
