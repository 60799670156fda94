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


def test_keep_scores_more_units_than_one_launch_holds_some_of_them_idle():
    """rtk_pivotkv_keep_scores_batched: 101 units of 1 to 40 kept rows and 10 idle ones (keep == 0, the last unit among them) in
    one call - two launches, the idle units take no slot of either - against score[keep_idx] in torch (keep_idx NULL:
    score[0 .. keep - 1]).  Every destination has two rows more than its unit keeps, which stay as they were."""
    import retake._native as nv

    n = nv.KEEP_SCORES_MAX_UNITS + 15
    g = torch.Generator(device="cpu")
    g.manual_seed(7)
    keeps = [0 if i % 12 == 2 or i == n - 1 else 1 + i % 40 for i in range(n)]
    assert keeps.count(0) == 10 and n - keeps.count(0) == nv.KEEP_SCORES_MAX_UNITS + 5
    scores = [torch.rand(64, generator=g) for _ in range(n)]
    idxs = [None if i % 7 == 3 else torch.randperm(64, generator=g)[:keep].sort().values for i, keep in enumerate(keeps)]
    dscores, didxs = [s.to(dev()) for s in scores], [None if x is None else x.to(dev()) for x in idxs]
    outs = [torch.full((keep + 2,), -7.0, device=dev()) for keep in keeps]
    arr = (nv.KeepScoresUnit * n)(*[nv.KeepScoresUnit(s.data_ptr(), None if x is None else x.data_ptr(), o.data_ptr(), keep)
                                    for s, x, o, keep in zip(dscores, didxs, outs, keeps)])
    nv.check(nv.lib.rtk_pivotkv_keep_scores_batched(arr, n, nv.stream()), "rtk_pivotkv_keep_scores_batched")
    torch.cuda.synchronize()
    for i, (s, x, o, keep) in enumerate(zip(scores, idxs, outs, keeps)):
        want = s[:keep] if x is None else s[x]
        assert torch.equal(o.cpu(), torch.cat([want, torch.full((2,), -7.0)])), i
