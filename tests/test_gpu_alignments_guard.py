"""The alignment stage under MDBG_GUARD (tests/test_gpu_guard.py has the method): one fresh process with the hook set runs the guard's self-test, then the
alignment tests as they are — the catalogue, the shapes at which the kernels can still go wrong, the ring, the ranges — while rust_mdbg_amd.api compares the bands of
every device block after every library call.  Every block is exactly as large as alignments.hip asked for, so a write one element past a column lands in a band."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT
from test_gpu_guard import GUARD_LINE

pytestmark = pytest.mark.gpu


def child_alignments(R):
    import sketch_graphs as G
    import test_gpu_alignments as TA
    for name in G.CASE_IDS:
        TA.test_catalogue_on_the_plain_and_on_every_simplified_list(name)
    TA.test_random_minimizer_space_graphs(6)
    TA.test_two_long_reads_cross_every_workgroup_span()
    for presimp, chained in ((0.0, True), (0.5, False)):
        TA.test_a_read_of_2101_steps_all_chained_or_none(presimp, chained)
    TA.test_short_reads_empty_reads_and_the_ends_of_a_range()
    TA.test_a_ring_of_four_entries_walked_two_and_a_half_times_on_either_strand()
    TA.test_an_alignment_is_cut_exactly_at_a_missing_key()
    TA.test_a_partition_into_three_ranges_concatenates(1)
    TA.test_base_space_and_a_batch_that_is_not_resident()


def test_alignments_under_guard():
    base = {k: v for k, v in os.environ.items() if k not in ("MDBG_GUARD", "MDBG_POISON")}
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_gpu_guard as T; import test_gpu_alignments_guard as A; "
            "T.CHILDREN['alignments'] = A.child_alignments; T.child_main('alignments')" % (ROOT, os.path.join(ROOT, "tests")))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(base, MDBG_GUARD="1"), timeout=600)
    print(r.stdout[-2500:])
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    got = GUARD_LINE.search(r.stdout)
    assert got is not None and r.stdout.startswith("SELFTEST_OK\n"), (r.stdout[-1500:], r.stderr[-3000:])
    assert int(got.group(1)) > 0 and int(got.group(2)) > 0
