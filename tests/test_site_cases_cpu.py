"""The planted columns of site_cases.py reach what they are planted for: asserted from the oracle's per-column statistics
(oracle_py.call_sites.stats), so that a changed builder cannot lose an edge quietly.  Conditions, not measurements.

What depends on threshold and theta is asserted under the run that can reach it, for a reason:
  * after a pass the list is cut 2.3 nats below its best configuration, so a second configuration has at least a tenth of the best one's
    weight and the sample in which they differ at most 1 / 1.1 = 0.909 < 0.95: under the defaults a list of two or more configurations
    always asks for a second pass (N >= 4), and a list of one whose carrier is called has no homozygous configuration.  "Kept by the small
    beam with two to four configurations", and the early and long-list rules as the ONLY reason, can therefore only occur below a
    threshold of 0.909: they are asserted under the run "weak_prior" (0.5, 0.5).
  * the cut at 514 configurations needs nine or more samples that each double the list; under theta = 0.001 a second allele costs 6.9
    nats and the planted shallow samples do not: asserted under "weak_prior" too."""
import numpy as np
import pytest

import oracle_py
import site_cases as sc


def _col(a, family, name):
    i = np.nonzero((a["family"] == family) & (a["name"] == name))[0]
    assert len(i) == 1, (family, name, len(i))
    return int(i[0])


def _tot(a):
    return a["reads"][:, :, :5].astype(np.int64).sum(2)


@pytest.mark.parametrize("N", sc.SIZES)
def test_builder_is_deterministic_and_mixed(N):
    a = sc.arrays(N)
    b = sc.cases(N)
    assert list(b) == list(sc.FAMILIES)
    assert all(np.array_equal(x[1], y[1]) for fam in sc.FAMILIES for x, y in zip(b[fam], sc.cases(N)[fam]))
    # planted and plain columns alternate: every piece of eight columns holds both kinds; two chunks of 256 columns at least
    assert len(a["dom"]) > 256
    for s in range(0, len(a["dom"]) - 7, 8):
        assert a["planted"][s:s + 8].any() and not a["planted"][s:s + 8].all()
    assert (a["dom"] > 3).sum() >= 4
    # one reference base for the whole builder, on request
    one = sc.cases(N, 2)
    assert all((r[:, 2] > 0).any() for fam in sc.FAMILIES for _, r, _ in one[fam][:3])


@pytest.mark.parametrize("N", sc.SIZES)
def test_depth_floor_filters_scale_and_table_edges(N):
    a = sc.arrays(N)
    tot = _tot(a)
    for run, md in (("default", 2), ("haploid", 1)):
        e = sc.expected(N, run)
        ran = e["passes"] >= 1
        # a sample is called exactly when it is above the floor, wherever a pass was run
        assert np.array_equal((e["call"] < 14)[ran], (tot > md)[ran])
        fam = (a["family"] == "depth_floor") & a["planted"] & ran
        alt = tot - a["reads"][np.arange(len(tot))[:, None], np.arange(N)[None, :], np.minimum(a["dom"], 3)[:, None]]
        for carrier in (False, True):
            m = fam[:, None] & ((alt > 0) == carrier)
            assert (m & (tot == md)).any() and (m & (tot == md + 1)).any(), (run, carrier)
    e = sc.expected(N)
    # site filters: 8 N - 1 reads are dropped, 8 N kept; fewer than half of the samples with 8 reads drop the column, but not on chrY
    n_drop = n_keep = 0
    for i in np.nonzero((a["family"] == "site_filters") & a["planted"])[0]:
        kind, v, c = str(a["name"][i]).split("_")
        chrom = int(c[1:])
        assert chrom == a["chrom"][i]
        if kind == "total":
            dropped = v == "8n-1"
            assert tot[i].sum() == (8 * N - 1 if dropped else 8 * N)
        else:
            assert (tot[i] >= 8).sum() == int(v) and tot[i].sum() >= 8 * N
            dropped = int(v) < 0.5 * N and (chrom & 3) != 2
        assert (e["passes"][i] == 0) == dropped, a["name"][i]
        n_drop += dropped
        n_keep += not dropped
    assert n_drop >= 6 and n_keep >= 6
    names = set(a["name"][(a["family"] == "site_filters")].tolist())
    h = (N + 1) // 2 - 1 if N % 2 else N // 2 - 1                     # the largest count that is below half
    assert {"count_%d_c0" % h, "count_%d_c2" % h, "count_%d_c16" % h, "count_%d_c18" % h, "count_%d_c0" % (h + 1)} <= names
    # scale and table edges: the depths are there, alone and in a carrier, and every such column is called
    for fam, depths in (("scale", (9, 10, 11, 99, 100, 101)), ("table_edges", (1446, 1447, 9999, 10000, 10001, 65535, 131070))):
        m = (a["family"] == fam) & a["planted"]
        assert (e["passes"][m] >= 1).all()
        nonref = ((e["call"] != a["dom"][:, None]) & (e["call"] < 14)).any(1)
        for d in depths:
            alone, beside = ("ref_%d" % d, "het_%d" % d) if fam == "scale" else ("%d_alone" % d, "%d_carrier" % d) if d < 70000 else ("65535x65535_alone", "65535x65535_carrier")
            i, j = _col(a, fam, alone), _col(a, fam, beside)
            assert (tot[i] == d).sum() == 1 and (tot[j] == d).sum() == 1 and (nonref[j] or N < 4) and (nonref[i] == (d > 70000)), (fam, d)
    assert a["reads"].max() == 65535
    # the head of the ln n! table: 1,446 reads stay under it, 1,447 do not (pcs_fast_kernel: every count + 601 >= 2048)
    deep = (a["reads"].astype(np.int64).sum(2) + 601 >= 2048).any(1)
    assert not deep[_col(a, "table_edges", "1446_alone")] and deep[_col(a, "table_edges", "1447_alone")]


@pytest.mark.parametrize("N", sc.SIZES)
def test_indel_support_and_types(N):
    a = sc.arrays(N)
    e = sc.expected(N)
    w = sc.expected(N, "weak_prior")
    # an indel genotype needs three reads of the indel
    for k, ok in ((2, False), (3, True)):
        for kind, gts in (("del", (4, 12)), ("ins", (5, 13))):
            for res in (e, w):
                for nm in ("%s_only_%d" % (kind, k), "%s_reads_%d" % (kind, k)):
                    assert not np.isin(res["call"][_col(a, "indel", nm)], gts).any() or ok, nm
    assert np.isin(w["call"][_col(a, "indel", "del_only_3")], (4, 12)).any() and np.isin(w["call"][_col(a, "indel", "ins_only_3")], (5, 13)).any()
    if N >= 8:
        for nm, g in (("het_del", 12), ("hom_del", 4), ("hom_ins", 5)):
            assert (e["call"][_col(a, "indel", nm)] == g).sum() == 1, nm
        assert e["stats"]["fallback"][_col(a, "indel", "all_hom_del")] & oracle_py.FALLBACK_INDEL
    t = {nm: int(e["type"][_col(a, "types", nm)]) for nm in a["name"][(a["family"] == "types") & a["planted"]]}
    tw = {nm: int(w["type"][_col(a, "types", nm)]) for nm in t}
    if N >= 8:
        assert (t["snp"], t["del"], t["ins"], t["hom_snp"], t["all_lanes"]) == (1, 2, 3, 1, 1), t
        assert t["multi_2"] == 5 and t["multi_3"] == 5 and t["multi_snp_del"] == 5
        # LOW on both sides of low_base, by its second argument (default run) and by its first (8 reads; all samples are shallow there and
        # only the weak prior's run calls the carrier with confidence at every N)
        assert (t["low_avg_at"], t["low_avg_above"]) == (4, 1) and (tw["low8_8"], tw["low8_9"]) == (4, 1), (t, tw)
        # MESS: an off-target share of exactly 0.15 is not above it
        assert t["mess_at"] == 1 and t["mess_over"] == 6
        tot = _tot(a)
        i = _col(a, "types", "mess_at")
        off = tot[i].sum() - a["reads"][i, :, a["dom"][i]].sum() + 0
        carrier = np.nonzero(e["call"][i] != a["dom"][i])[0]
        assert len(carrier) == 1 and 20 * (off - tot[i, carrier[0]]) == 3 * tot[i].sum()
    if N >= 64:
        planted = a["planted"]
        assert set(range(1, 7)) <= set(e["type"][planted].tolist())
        # a confident carrier in every lane of lanes(N)
        conf = (e["call"] != a["dom"][:, None]) & (e["call"] < 14) & (e["p"] >= 0.95)
        assert conf[_col(a, "types", "all_lanes")].sum() == len(sc.lanes(N))
        assert all(conf[planted][:, i].sum() >= 3 for i in sc.lanes(N))


@pytest.mark.parametrize("N", [n for n in sc.SIZES if n >= 8])
def test_small_beam_rules_passes_and_ties(N):
    a = sc.arrays(N)
    U = sc.maxu(N)
    runs = {r: sc.expected(N, r) for r in ("default", "weak_prior")}
    st = runs["default"]["stats"]
    # exactly MAXU and MAXU + 1 unsettled samples, nothing else the matter
    h = sc.hand_off(N, st)
    others = h["early"] | h["long"] | h["no_hom"] | h["changed"]
    for n, handed in ((U, False), (U + 1, True)):
        i = _col(a, "small_beam", "weak_%d" % n)
        assert st["unset"][i] == n and not others[i] and h["many"][i] == handed
    # every hand-off rule is the only reason for a column, in one of the runs (module docstring)
    only = {}
    for r, e in runs.items():
        hh = sc.hand_off(N, e["stats"])
        rules = ("many", "early", "long", "no_hom", "changed")
        for k in rules:
            alone = hh[k] & ~np.any([hh[q] for q in rules if q != k], axis=0)
            only[r, k] = a["name"][alone & a["planted"]].tolist()
    assert only["default", "many"] and only["default", "changed"] and only["weak_prior", "early"] and only["weak_prior", "long"]
    assert only["weak_prior", "no_hom"], only
    assert "early_soft" in only["weak_prior", "early"] and "soft_3_alleles_ref_8" in only["weak_prior", "long"]
    # the list before the last expansions: four (kept) and five (handed off); a column the small beam keeps with two to four configurations
    ws = runs["weak_prior"]["stats"]
    wh = sc.hand_off(N, ws)
    kept = wh["live"] & ~(wh["many"] | wh["early"] | wh["long"] | wh["no_hom"] | wh["changed"])
    assert (ws["pre_list"][kept] == 4).any() and (ws["pre_list"] == 5).any()
    assert ((ws["max_list"][kept] >= 2) & (ws["max_list"][kept] <= 4)).any()
    assert kept[_col(a, "small_beam", "soft_2")] and kept[_col(a, "small_beam", "soft_3_alleles")]
    # an unsettled carrier ahead of a settled sample
    assert st["early"][_col(a, "small_beam", "early_het")] == 1 and st["early"][_col(a, "types", "snp")] == 1
    # passes
    assert {0, 1, 2, 5} <= set(runs["default"]["passes"][a["planted"]].tolist())
    # ties: equal margins in the planted family, equal posteriors somewhere; the fallback with and without its second sort
    fam = (a["family"] == "ties") & a["planted"]
    assert ((st["margin_tie"][fam] & 1) > 0).all()
    assert st["unset"][_col(a, "ties", "weak_x4")] == 4 and st["unset"][_col(a, "ties", "het_x4")] == 4
    assert (st["post_tie"][a["planted"]] > 0).any() and (ws["post_tie"][fam] > 0).any()
    fb = st["fallback"][a["planted"]]
    assert ((fb & 1) > 0).any() and ((fb & oracle_py.FALLBACK_INDEL) > 0).any()
    if N >= 64:
        i = _col(a, "small_beam", "shallow_x16")
        assert ws["cut"][i] == 1 and ws["max_list"][i] > 514 and ws["post_tie"][i] == 1


def test_single_pass_rule_below_four_samples():
    a = sc.arrays(3)
    e = sc.expected(3)
    assert e["passes"].max() == 1 and (e["passes"] == 0).any()
    # ... where the same columns of 8 samples take more
    assert sc.expected(8)["passes"].max() == 5
    # with one pass a list of several configurations ends the column: the small beam keeps what it hands off at N >= 4
    h = sc.hand_off(3, e["stats"])
    assert not h["changed"].any() and (h["live"] & (e["stats"]["max_list"] >= 2) & ~h["no_hom"] & ~h["early"]).any()


@pytest.mark.parametrize("N", [8, 129])
@pytest.mark.parametrize("run", list(sc.REFERENCE_RUNS))
def test_site_oracle_matches_reference_text_on_planted_columns(N, run):
    """the oracle against the rows the reference itself printed for the planted columns (tests/golden/pecall_edges*), .base and .snp, row
    for row; the fixture holds the builder's columns of today"""
    f = sc.reference(N)
    planted = [r for cols in sc.cases(N).values() for _, r, _ in cols]
    assert len(planted) == len(f["pos"])
    call, p, typ, ac, _ = oracle_py.call_sites(f["reads"], f["dom"], **sc.REFERENCE_RUNS[run])
    assert sorted(np.array(planted).sum(1).tolist()) == sorted(f["reads"].astype(np.int64).sum(1).tolist())
    assert set(typ.tolist()) >= ({0, 1, 2, 3, 4, 5, 6} if run == "" else {0, 1})
    bad = sc.reference_mismatches(N, run, call, p, typ, ac)
    assert not bad, (len(bad), bad[:2])
