"""The chain stage under MDBG_GUARD (tests/test_gpu_guard.py has the method): one fresh process with the hook set runs the guard's self-test, then the chain tests
as they are — the hand-built cases, a random graph with mutated reads, the read of 2,101 alignments, the ranges, base space through chain_batch — while
rust_mdbg_amd.api compares the bands of every device block after every library call.  Every block is exactly as large as chains.hip asked for, so a write one
element past a column lands in a band."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT
from test_gpu_guard import GUARD_LINE

pytestmark = pytest.mark.gpu


def child_chains(R):
    import chain_graphs as CG
    import test_gpu_chains as TC
    for name in CG.CASE_IDS:
        TC.test_hand_built_cases(name)
    TC.test_random_graphs_with_mutated_reads(4)
    TC.test_a_read_of_2101_alignments_all_bridged_or_none()
    TC.test_a_partition_into_three_ranges_concatenates_and_the_ends_of_a_range()
    TC.test_base_space_planted_substitutions_and_a_batch_that_is_not_resident()
    TC.test_chain_batch_on_a_genome_with_a_repeat_and_a_ring()


def test_chains_under_guard():
    base = {k: v for k, v in os.environ.items() if k not in ("MDBG_GUARD", "MDBG_POISON")}
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_gpu_guard as T; import test_gpu_chains_guard as A; "
            "T.CHILDREN['chains'] = A.child_chains; T.child_main('chains')" % (ROOT, os.path.join(ROOT, "tests")))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(base, MDBG_GUARD="1"), timeout=600)
    print(r.stdout[-2500:])
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    got = GUARD_LINE.search(r.stdout)
    assert got is not None and r.stdout.startswith("SELFTEST_OK\n"), (r.stdout[-1500:], r.stderr[-3000:])
    assert int(got.group(1)) > 0 and int(got.group(2)) > 0
