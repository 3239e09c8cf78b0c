"""The host pipeline that feeds the mapper's kernels (run_slice, ring_setup, ensure_work of pemap_capi.hip) where no other test takes it:
runs of several chunks that continue a pending pipeline, the table of 256 chunks filled and exceeded, the longest read changing between
batches in flight, the ring re-made with mixed lengths in flight, parameters changed and the pileup reset with batches in flight.  The
plans are tests/seam_cases.py (what they reach: tests/test_seam_cases_cpu.py), the drivers tests/seam_gpu_worker.py.  Expected: exact
equality with the reference's golden outputs (r150 plans) and with the oracle (ragged plans), and from pemap_dev_pipeline_stats the path
every submit took.

With pemap_dev_set_params as it was (values stored at once, whatever is in flight) the two `params` tests fail on the device: in
test_params_change_behind_batches_in_flight the first paired batch comes back with m2 all zero, in
test_max_dist_change_before_the_wait the summary is folded under the later limit (total_dist 28,181 over 127 pairs where the oracle has
31,089 over 134)."""
import os
import subprocess
import sys
import pytest
import seam_gpu_worker as w

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def dev():
    d = w.make_dev()
    yield d
    d.close()


# the knobs are read when an object is made: one child process per setting
@pytest.mark.parametrize("which,extra", [("A", {}), ("B", {"PEMAP_REPLICAS": "0"}), ("C", {"PEMAP_PIPELINE": "2"})])
def test_plans_at_chunks_of_64_pairs(which, extra):
    """A: uneven, exact_fill, one_run, lengths on one object; B: uneven and lengths on the reference's table layout (the lists in HBM,
    vote, remainder and emit on the ALU stream: ev_lists_free carries real work); C: uneven on one stream, where nothing continues"""
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.dirname(HERE), HERE]), PEMAP_CHUNK_PAIRS="64", **extra)
    r = subprocess.run([sys.executable, os.path.join(HERE, "seam_gpu_worker.py"), which], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    print(r.stdout.decode(errors="replace")[-3000:])
    assert r.returncode == 0 and ("seam ok " + which).encode() in r.stdout, (which, r.returncode, r.stdout[-3000:])


def test_longest_read_moves_between_batches_in_flight(dev):
    """default knobs: every batch is one chunk, only the geometry moves"""
    print("counters lengths", w.plan_lengths(dev, one_chunk=True))


def test_ring_remade_with_mixed_lengths_in_flight(dev):
    print("counters remade", w.plan_remade(dev))


def test_params_change_behind_batches_in_flight(dev):
    w.plan_params(dev)


def test_max_dist_change_before_the_wait(dev):
    w.plan_params_dist(dev)


def test_reset_pileup_is_refused_with_a_batch_in_flight(dev):
    w.plan_reset_refused(dev)
