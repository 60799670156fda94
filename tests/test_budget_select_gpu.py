"""rtk_pivotkv_budget_select_batched alone, straight through the C ABI, against the rule's CPU restatement
(tests/budget_ref.py: a stable descending sort).  Per unit: the newest row always, and an exact top-(keep - 1) of the others,
ties to the lowest index; the output is an ascending int32 list.  Every (n, keep) of a score pattern travels in ONE call -
units of different n in one launch.  n lies on both sides of the workgroup's 1024 threads and of the 16 384 keys the LDS form
of the chunk selection holds."""
import pytest
import torch

import budget_ref as br

pytestmark = pytest.mark.gpu

NS = (1, 2, 1023, 1024, 1025, 16384, 16385, 40000)


def dev():
    return torch.device("cuda:0")


def _scores(kind, n, seed):
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    if kind == "all_equal":
        return torch.full((n,), 0.7)
    if kind == "four_values":
        return torch.tensor([0.25, 0.5, 1.0, 2.0])[torch.randint(0, 4, (n,), generator=g)]
    if kind == "many_ones":        # key-patch rows at exactly 1.0 among values above and below
        s = torch.rand(n, generator=g) * 2.0
        s[torch.rand(n, generator=g) < 0.3] = 1.0
        return s
    assert kind == "last_is_minimum"
    s = torch.rand(n, generator=g) + 1.0
    s[n - 1] = 0.0
    return s


def _cases():
    return [(n, keep) for n in NS for keep in sorted({1, 2, n - 1, n}) if 1 <= keep <= n]


def _select(units):
    """units: [(scores on the CPU, keep)] -> the int32 lists of one call."""
    import retake._native as nv

    dscores = [s.to(dev()) for s, _ in units]
    outs = [torch.full((keep,), -7, dtype=torch.int32, device=dev()) for _, keep in units]
    arr = (nv.BudgetSelectUnit * len(units))(*[nv.BudgetSelectUnit(s.data_ptr(), o.data_ptr(), s.numel(), o.numel())
                                               for s, o in zip(dscores, outs)])
    nv.check(nv.lib.rtk_pivotkv_budget_select_batched(arr, len(units), nv.stream()), "rtk_pivotkv_budget_select_batched")
    torch.cuda.synchronize()
    return [o.cpu() for o in outs]


@pytest.mark.parametrize("kind", ["all_equal", "four_values", "many_ones", "last_is_minimum"])
def test_against_the_stable_sort(kind):
    cases = _cases()
    assert len(cases) <= 96                              # one launch
    units = [(_scores(kind, n, 100 * i + n), keep) for i, (n, keep) in enumerate(cases)]
    for (n, keep), (s, _), got in zip(cases, units, _select(units)):
        assert got.dtype == torch.int32 and got.shape == (keep,)
        want = br.survivors(s, keep)
        assert torch.equal(got.long(), want), (kind, n, keep)
        assert int(got[-1]) == n - 1                     # the newest row survives - also where it holds the minimum
        assert bool((got[1:] > got[:-1]).all())          # ascending
        if keep == n:
            assert torch.equal(got.long(), torch.arange(n))


def test_more_units_than_one_launch_holds():
    import retake._native as nv

    units = [(_scores("many_ones", 50 + i, i), 1 + i % 40) for i in range(nv.BUDGET_SELECT_MAX_UNITS + 5)]
    for (s, keep), got in zip(units, _select(units)):
        assert torch.equal(got.long(), br.survivors(s, keep))
