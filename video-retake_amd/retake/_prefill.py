"""Model-independent pieces of ReTaKe's chunked prefill (shared by the Qwen2-VL and LLaVA-Video glue).

Reference: retake/qwen2_vl.py:444-475 (segment_input_ids), :548-557 (dynamic ratio), :670-720 (chunked
prefill loop); retake/llava_onevision.py:164-198, :337-347, :499-545 are the same logic for LLaVA.
"""
from __future__ import annotations

import math
from typing import Callable, List, Optional, Tuple

import torch

Segment = Tuple[int, int, str]


def segment_token_runs(is_video: torch.Tensor) -> List[Segment]:
    """Run-length segmentation of a 1-D bool tensor into sorted (start, end, 'video' | 'text') runs,
    end exclusive (reference: qwen2_vl.py:444-475)."""
    flags = is_video.to(torch.bool).cpu().tolist()
    segments: List[Segment] = []
    start = 0
    for i in range(1, len(flags) + 1):
        if i == len(flags) or flags[i] != flags[start]:
            segments.append((start, i, "video" if flags[start] else "text"))
            start = i
    return segments


def apply_dynamic_compression_ratio(config, input_length: int) -> None:
    """`dynamic_compression_ratio`: ratio = max_input_length / input_length when the prompt is longer than
    the budget, else 1.  Written back into the shared config dict (reference: qwen2_vl.py:548-557)."""
    kwargs = getattr(config, "longvideo_kwargs", None)
    if not kwargs or not kwargs.get("kvcache_compression", False):
        return
    comp = kwargs["kvcache_compression_kwargs"]
    if comp.get("dynamic_compression_ratio", False):
        max_len = comp["max_input_length"]
        comp["compression_ratio"] = 1 if input_length <= max_len else max_len / input_length


def expected_cache_tokens(config, input_length: int, chunk_size: Optional[int]) -> Optional[int]:
    """Capacity hint for the pre-allocated PivotKV cache (not in the reference): the prompt compressed at the configured
    ratio, plus one uncompressed chunk in flight, plus room for generation.  An over-long answer only costs a regrowth."""
    kwargs = getattr(config, "longvideo_kwargs", None)
    if not kwargs or not kwargs.get("kvcache_compression", False) or chunk_size is None:
        return None
    ratio = float(kwargs["kvcache_compression_kwargs"].get("compression_ratio", 1.0))
    return int(math.ceil(min(1.0, ratio) * input_length)) + int(chunk_size) + 2048


def cache_reserves(config, input_length: int, chunk_size: Optional[int], segments: Optional[List[Segment]] = None) -> dict:
    """Keyword arguments for build_kvcache: `reserve_tokens` as expected_cache_tokens gives it - or, with
    longvideo_kwargs["kv_cache_dtype"] = "fp8_e4m3", where the kept video rows live in the fp8 archive and the 16-bit
    buffers hold only what is not one: reserve_archive_tokens = ceil(ratio x video tokens) and reserve_tokens = the
    non-video prompt tokens + one chunk in flight + room for generation.  `segments`: segment_token_runs of the prompt."""
    out = {"reserve_tokens": expected_cache_tokens(config, input_length, chunk_size)}
    kwargs = getattr(config, "longvideo_kwargs", None)
    if out["reserve_tokens"] is None or not kwargs.get("kv_cache_dtype") or segments is None:
        return out
    video = sum(e - s for s, e, kind in segments if kind == "video")
    ratio = float(kwargs["kvcache_compression_kwargs"].get("compression_ratio", 1.0))
    out["reserve_archive_tokens"] = int(math.ceil(min(1.0, ratio) * video))
    out["reserve_tokens"] = (input_length - video) + int(chunk_size) + 2048
    return out


def prompt_guided(config) -> bool:
    kwargs = getattr(config, "longvideo_kwargs", None)
    if not kwargs or not kwargs.get("kvcache_compression", False):
        return False
    comp = kwargs["kvcache_compression_kwargs"]
    return bool(comp.get("prompt_guided_compression", False) and comp.get("compression_ratio", 1) < 1.0)


def followup_position_ids(mark, n: int, device=None) -> torch.Tensor:
    """Position ids of `n` text rows appended where the video ended (not in the reference, which prefills the video again
    for every question): `mark.resume_position_ids + arange(n)` on every row, as [3, 1, n] (M-RoPE) or [1, n] int64 on
    `device` - the ids a fresh prefill would have given n text rows at that place.  `mark` is `cache.video_end` after a
    chunked prefill.  The attention patches then shift the temporal row by their continuity rule, as for any segment."""
    resume = getattr(mark, "resume_position_ids", None)
    if resume is None:
        raise ValueError("followup_position_ids: the mark carries no resume_position_ids (it is not the `video_end` of a "
                         "chunked prefill whose video was followed by text)")
    P = resume.numel()
    if P not in (1, 3):
        raise ValueError(f"followup_position_ids: resume_position_ids must hold 1 or 3 ids, got {P}")
    ids = resume.to(torch.int64).reshape(P, 1) + torch.arange(int(n), dtype=torch.int64)
    ids = ids.reshape(3, 1, int(n)) if P == 3 else ids
    return ids if device is None else ids.to(device)


def run_chunked_prefill(segments: List[Segment], chunk_size: int, cache, keypatches_mask,
                        run_text: Callable[[int, int], object], run_video_chunk: Callable[[int, int], object],
                        position_ids: Optional[torch.Tensor] = None):
    """The prefill driver (reference: qwen2_vl.py:670-720).

    Text segments are prefilled in one call with compression off; each video segment is cut into
    `chunk_size`-token chunks, the cache gets the chunk's key-patch mask (the callback fires the
    `before_forward` / `after_forward` hooks around the model call), and compression is switched off
    again afterwards so that decoding appends normally.  Returns the last model output.

    position_ids (not in the reference): the forward's ids of the whole prompt, [3, 1, S] or [1, S].  Before the text
    segment that follows the last video run is prefilled, the ids of its first row - as the forward computed them, before
    the attention patch shifts them - are noted on `cache.video_end` (a cache with `mark` only; followup_position_ids).
    """
    compression_on = getattr(cache, "kvcache_compression", False)
    outputs = None
    last_video = max((i for i, seg in enumerate(segments) if seg[2] == "video"), default=None)
    for i, (s, e, kind) in enumerate(segments):
        if kind == "text":
            # (with visual compression the reference segments the prompt BEFORE the video tokens are dropped: the runs then
            # do not line up with the ids, the trailing text is prefilled inside the last "video" chunks, nothing is noted)
            if last_video is not None and i == last_video + 1 and position_ids is not None and hasattr(cache, "mark") \
                    and cache.video_end is not None and s < e and segments[-1][1] == position_ids.shape[-1]:
                cache.set_resume_position_ids(position_ids[..., s])
            cache.kvcache_compression = False
            outputs = run_text(s, e)
        elif kind == "video":
            cache.kvcache_compression = compression_on
            for idx in range(math.ceil((e - s) / chunk_size)):
                ss = s + idx * chunk_size
                ee = min(s + (idx + 1) * chunk_size, e)
                if keypatches_mask is not None:
                    cache.keypatches_mask_chunk = keypatches_mask[0, ss:ee]
                outputs = run_video_chunk(ss, ee)
            cache.keypatches_mask_chunk = None
            cache.kvcache_compression = False  # turned off for decoding
        else:
            raise ValueError(kind)
        try:  # the model hands the cache back through its output (reference: `past_key_values = outputs[...]`)
            cache = outputs["past_key_values"]
        except (KeyError, TypeError, IndexError):
            pass
    return outputs
