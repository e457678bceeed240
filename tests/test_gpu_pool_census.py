"""The pool's host-buffer paths make the calls and return the bits they did before the pool's sources were split (GPU, -m gpu):
tests/pool_census.py walks its script on the smallest pool of each path — zero-copy with the completion word written by the kernel, by
the queue, or not at all; a one-launch pass over several streams; a pass of several launches; pinned staging with copies both ways —
and every step's table of HIP runtime calls and every output's sha256 must equal tests/golden/pool_census.json, which was recorded three
times on the commit before the split (the file names what the recordings disagreed on and leaves only that out). The table is the test
build's (aidax_test_hip_calls): the shipped library has none, so this runs on the test build only; the check of the
committed file itself needs no GPU."""
import json
import os

import pytest

from tests import conftest, pool_census


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(conftest.GOLDEN, "pool_census.json")) as f:
        return json.load(f)


def test_the_golden_census_covers_every_host_path_and_drops_only_what_a_poll_may_add(golden):
    pools = golden["pools"]
    assert list(pools) == [name for name, *_ in pool_census.POOLS] and golden["recordings"] == 3
    for d in golden["dropped"]:
        assert d["call"] in pool_census.MAY_VARY and d["step"].split(" ", 1)[1].split(" of ")[0] in pool_census.MAY_VARY_IN, d
    first = lambda name: next(s for s in pools[name] if s["step"].endswith(" process"))["calls"]
    assert "hipStreamWriteValue32" not in first("zc_kernel_word") and "hipMemcpyAsync" not in first("zc_kernel_word")      # the kernel's own word
    assert first("zc_queue_word").get("hipStreamWriteValue32") == 1 and first("zc_five").get("hipStreamWriteValue32") == 1
    assert first("zc_no_word").get("hipStreamSynchronize") == 1 and "hipStreamWriteValue32" not in first("zc_no_word")
    assert first("zc_multi_launch").get("hipMemcpyAsync") == 1                # several launches: the download from the device block
    assert first("staged").get("hipMemcpyAsync") == 2                          # copies both ways
    for steps in pools.values():
        assert all(len(s["out"]) == 1 for s in steps if s["step"].split(" ", 1)[1].split(" of ")[0] in ("process", "collect", "read_meters with clear", "read_gate"))


@pytest.mark.gpu
def test_every_step_makes_the_recorded_calls_and_returns_the_recorded_bits(golden):
    if conftest.SHIP_LEG:
        pytest.skip("aidax_test_hip_calls: a test hook — the shipped library has none")
    bad = pool_census.differences(golden, pool_census.run())
    assert not bad, "\n".join(bad)
