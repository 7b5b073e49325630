"""alloc_sweep.verdict, the end of every allocation-failure sweep, on synthetic tallies: no library, no GPU."""
import pytest

from alloc_sweep import Case, verdict


def case(**end):
    return Case("synthetic", None, None, None, None, **end)


PLAIN = case()
AUTO = case(auto=True, flags={"flow": 0})
STRICT = case(min_failed=lambda cold: cold - 1, max_retried=1, retried_only_at=1, strict_requests=True)


def test_consistent_tallies_pass():
    verdict(PLAIN, 4, [1, 2, 4], [], [(3, 4)])               # (not strict: an armed call may succeed with fewer requests)
    verdict(AUTO, 4, [], [1, 2, 4], [(3, 5)])
    verdict(STRICT, 4, [2, 3, 4], [], [(1, 5)])
    verdict(STRICT, 4, [1, 2, 3, 4], [], [])


@pytest.mark.parametrize("c,failed,fell_back,retried,message", [
    pytest.param(PLAIN, [1, 2, 4], [], [], "not every one", id="a-k-missing"),
    pytest.param(AUTO, [], [1, 2], [(3, 5)], "not every one", id="a-k-missing-auto"),
    pytest.param(case(max_retried=1), [3, 4], [], [(1, 5), (2, 5)], "at most 1 may", id="more-retried-than-max_retried"),
    pytest.param(STRICT, [2, 3, 4], [], [(1, 6)], "a cold call makes 4", id="cold-plus-2-requests-under-strict_requests"),
    pytest.param(AUTO, [2], [1, 4], [(3, 5)], "returned BSPGEMM_ERR_ALLOC", id="auto-with-a-failed-k"),
    pytest.param(AUTO, [], [], [(1, 5), (2, 5), (3, 5), (4, 5)], "no k showed", id="auto-without-a-fallback"),
    pytest.param(PLAIN, [], [], [(1, 5), (2, 5), (3, 5), (4, 5)], "no k ended", id="plain-with-no-failed-k"),
    pytest.param(STRICT, [1, 3, 4], [], [(2, 5)], "only k = 1 may", id="retried_only_at-violated"),
    pytest.param(case(min_failed=4), [1, 2, 3], [], [(4, 5)], "at least 4 must", id="fewer-failed-than-min_failed"),
])
def test_inconsistent_tallies_raise(c, failed, fell_back, retried, message):
    with pytest.raises(AssertionError, match=message):
        verdict(c, 4, failed, fell_back, retried)
