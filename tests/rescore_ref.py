"""The budget's re-scoring rule (video_budget_rescore / video_budget_observe_rows), restated in float64 torch: the
specification rtk_pivotkv_rescore_batched and retake._video_bound.rescore_budget are tested against.  The rule is this
project's own - the reference processes a finished video and has no counterpart.

A layer's video region holds n rows; n_old of them existed at the last re-scoring.  With Q [Hq, Wc, D] the last Wc rotated
query rows of the layer's newest chunk, K [Hkv, >= n_old, D] the region's stored (rotated) keys and G = Hq // Hkv:

    p_h[i, .] = softmax over j < n_old of (Q[h, i] . K[h // G, j] / sqrt(D))     no mask; rows >= n_old are never read
    mass[j]   = (1 / Hq) sum_h sum_{i < Wc} p_h[i, j]                            sum_j mass[j] = Wc
    obs[j]    = mass[j] n_old / Wc                                               averages exactly 1 over the old rows
    score[j]  = (1 - alpha) score[j] + alpha obs[j]    j < n_old; rows >= n_old keep their arrival score

The library's fp32 form of the last line is fmaf(alpha, obs, (1 - alpha) * old): 1 - alpha rounded once, one product, one
fused multiply-add; its obs is (the fp32 sum of the probabilities) * ((float)n_old / (float)(Hq Wc)).

Bookkeeping (`Seen`): n_old is 0 at first (the first chunk does nothing), the region's rows after a re-scoring, the budget
after an eviction, and a rewind caps it at the restored number of scored rows."""
import torch


def mass(q: torch.Tensor, k: torch.Tensor, n_old: int) -> torch.Tensor:
    """float64 [n_old]."""
    Hq, Wc, D = q.shape
    Hkv = k.shape[0]
    G = Hq // Hkv
    q64 = q.detach().double().reshape(Hkv, G * Wc, D)
    k64 = k.detach()[:, :n_old].double()
    p = torch.softmax(q64 @ k64.transpose(1, 2) / float(D) ** 0.5, dim=-1)   # [Hkv, G Wc, n_old]
    return p.sum(dim=(0, 1)) / Hq


def obs(q, k, n_old: int) -> torch.Tensor:
    return mass(q, k, n_old) * n_old / q.shape[1]


def blend(old: torch.Tensor, observed: torch.Tensor, alpha: float) -> torch.Tensor:
    return (1.0 - alpha) * old.detach().double() + alpha * observed


def rescored(scores: torch.Tensor, q, k, n_old: int, alpha: float) -> torch.Tensor:
    """float64 scores [len(scores)] after one re-scoring: the first n_old blended, the rest as they were."""
    out = scores.detach().double().clone()
    if n_old > 0:
        out[:n_old] = blend(scores[:n_old].to(q.device), obs(q, k, n_old), alpha).to(out.device)
    return out


def bar(alpha: float, n_old: int, Wc: int, score_bar: float, mass64: torch.Tensor, want64: torch.Tensor) -> torch.Tensor:
    """Per row: alpha (n / Wc) BAR max(1, mass64[j]) + 4 2^-24 |want64[j]|.  BAR is the project's score bar (5e-6 for fp32
    operands, 2e-5 for 16-bit ones), set on column sums of magnitude about 1 - hence the max(1, .); a blended score is
    alpha n / Wc times such a sum plus two fp32 roundings of a value of want's size."""
    return alpha * (n_old / Wc) * score_bar * torch.clamp(mass64, min=1.0) + 4 * 2.0 ** -24 * want64.abs()


class Seen:
    """The per-layer count of rows the next re-scoring treats as old."""

    def __init__(self):
        self.n_old = 0

    def rescore(self, n: int) -> int:
        """A re-scoring of a region of n rows: returns the n_old it uses."""
        n_old, self.n_old = min(self.n_old, n), n
        return n_old

    def evict(self, B: int):
        self.n_old = B

    def rewind(self, sc_len: int):
        self.n_old = min(self.n_old, sc_len)
