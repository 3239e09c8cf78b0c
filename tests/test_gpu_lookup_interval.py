"""run_stats' `lookup` time.  The fused seed kernel's first tier stamps its own interval (workgroup 0 at entry, every wave at exit,
in fields zeroed with the chunk's counters); the second-tier-only schedule (PEMAP_FIRST_TIER=0) and the reference layout
(PEMAP_REPLICAS=0) keep their events.  In every form: a positive time, no longer than the seed stage it is part of, and the seed
stage shorter than the call that ran it -- in a second run on the same object as in the first.
"""
import time

import pytest

import pair_cases as pc

pytestmark = pytest.mark.gpu


def _run_twice(env, monkeypatch):
    from pecaller_amd import PemapDev
    for k, v in env.items():
        monkeypatch.setenv(k, v)           # the knobs are read by pemap_dev_create, once per object
    d = PemapDev(0)
    try:
        ix = pc.index()
        d.build_index(ix["genome"], ix["contig_len"])
        d.set_params(paired=True, min_dist=0, max_dist=500, min_align=0.85)
        batch = pc.reads(100)
        out = []
        for _ in range(2):
            t0 = time.perf_counter()
            d.map_batch(*batch)
            wall_ms = (time.perf_counter() - t0) * 1e3
            stats, times = d.run_stats()
            out.append((times, wall_ms, stats))
        return out, d.lookup_replicas()[0]
    finally:
        d.close()


def test_first_tier_stamps_its_interval(monkeypatch):
    runs, replicas = _run_twice({}, monkeypatch)
    assert replicas == 8
    for times, wall_ms, stats in runs:
        print(times, wall_ms)
        # (the stamps are zeroed per run: a second run's interval that began with the first run's stamp would be longer than its call)
        assert 0.0 < times["lookup"] <= times["seed"] < wall_ms, (times, wall_ms)
        # the scale of the clock: a launch of the persistent first tier over 6,000 ends is no shorter than the 20 us of a kernel
        # launch, and is one of a dozen kernels of a call that also copies the reads in and the results out
        assert 0.02 <= times["lookup"] <= wall_ms / 2, (times, wall_ms)


@pytest.mark.parametrize("env", [{"PEMAP_FIRST_TIER": "0"}, {"PEMAP_REPLICAS": "0"}], ids=["second_tier_only", "no_replicas"])
def test_the_other_schedules_keep_their_events(env, monkeypatch):
    runs, replicas = _run_twice(env, monkeypatch)
    assert replicas == (0 if "PEMAP_REPLICAS" in env else 8)
    for times, wall_ms, stats in runs:
        print(env, times, wall_ms)
        assert 0.0 < times["lookup"] <= times["seed"] < wall_ms, (env, times, wall_ms)
