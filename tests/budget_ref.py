"""The video budget's rule (video_budget_rows / video_budget_slack), restated on the CPU in torch: the specification the
HIP selection (rtk_pivotkv_budget_select_batched) and retake._video_bound.evict_budget are tested against.

A layer's video region holds n rows in sequence order, each with one fp32 score.  When n > B + S the region is evicted down
to B rows: the NEWEST row always survives, and of the other n - 1 rows the B - 1 with the highest score, ties to the lowest
index (a stable descending sort).  Survivors stay in sequence order."""
import torch


def survivors(scores: torch.Tensor, B: int) -> torch.Tensor:
    """Ascending int64 indices of the B rows of `scores` [n] that survive an eviction (n >= B >= 1)."""
    n = scores.numel()
    assert 1 <= B <= n
    order = torch.sort(scores[:n - 1].detach().float().cpu(), descending=True, stable=True).indices[:B - 1]
    return torch.cat([order.sort().values, torch.tensor([n - 1], dtype=torch.int64)])


def evict(scores: torch.Tensor, B: int, S: int = 0):
    """The rule as `after_forward` applies it: ascending indices of the rows that stay, or None when n <= B + S (nothing
    happens)."""
    return survivors(scores, B) if scores.numel() > B + S else None


def simulate(chunks, B: int, S: int = 0):
    """Feed chunks of kept-row scores (1-D tensors, in arrival order) to one region.  Returns, per chunk, (alive, dropped,
    evictions): the indices of the surviving rows INTO THE CONCATENATION of all chunks so far (what an unbounded twin
    holds), the rows dropped so far and the evictions so far."""
    alive = torch.empty(0, dtype=torch.int64)
    everything = torch.empty(0, dtype=torch.float32)
    dropped = evictions = 0
    out = []
    for c in chunks:
        c = c.detach().float().cpu()
        alive = torch.cat([alive, torch.arange(everything.numel(), everything.numel() + c.numel())])
        everything = torch.cat([everything, c])
        keep = evict(everything[alive], B, S)
        if keep is not None:
            dropped += alive.numel() - B
            evictions += 1
            alive = alive[keep]
        out.append((alive.clone(), dropped, evictions))
    return out
