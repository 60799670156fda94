"""PivotKVCache's methods live in several modules (retake/_flush.py, _update_stages.py, _marks.py, _focus.py,
_video_bound.py) and are bound in the class body, so a name can be lost or renamed without any definition failing: the
class has exactly the methods, properties and class-level defaults listed here, the module exports exactly its `__all__`,
and the user-facing methods carry docstrings (`help(PivotKVCache.fork)` is their documentation)."""
import pytest

# sorted(n for n in dir(PivotKVCache) if n not in dir(DynamicCache))
SURFACE = [
    "_STATIC_ROPE_TYPES", "_adopt", "_advance_layers", "_after_rewind", "_append_tail", "_archive", "_archive_reserve",
    "_bind_rotary", "_bind_update", "_bound_rotary", "_branch_check", "_branch_refuse_write", "_branch_update_check",
    "_branches", "_buf", "_check_mark", "_claim_slot", "_compact", "_compressed_in_forward", "_crop_floor", "_dead_marks",
    "_dense", "_end_flush", "_entry_guard", "_epoch", "_evict_staged", "_flush", "_flush_c", "_flush_general", "_flushes",
    "_fork_dead", "_fp8_refuse", "_fused_prepare", "_get_batch", "_ids_2d", "_keep_scores", "_kill_marks_after",
    "_mark_is_dead", "_mark_serial", "_new_id_tables", "_next_layer_prev", "_next_side", "_order_compaction", "_pos_reserve",
    "_pos_view", "_prompt_rows", "_region_room", "_reset_compaction", "_rope_tables", "_rotary", "_run_on_worker",
    "_run_stages", "_scan_unit", "_score_prompt_run", "_score_stage", "_score_unscored", "_score_ws_pointer",
    "_scores_q0_in_place", "_select_prompt_units", "_select_units", "_select_unselected", "_shift_failed",
    "_shift_latch_check", "_shift_pending_ids", "_shift_row", "_stage_passes", "_stage_post", "_stage_pre", "_store",
    "_take_mark", "_update_c", "_update_general", "_wait_workers", "_warn_compression", "_watch", "after_forward",
    "append_pre_rope", "archive", "archive_len", "attention", "before_forward", "check", "crop", "focus", "focus_kept",
    "focus_scores", "focused_from", "fork", "forked_from", "get_prev_temporal_idx", "key_cache", "last_compressed_mark",
    "last_keep_indices", "last_scores", "mark", "memory_footprint", "observed_queries", "position_cache", "position_offset",
    "reserve", "rewind", "row_scores", "set_resume_position_ids", "shared", "shared_len", "shift_temporal_ids_",
    "unwatch_question", "update_num_evicted_tokens", "update_position_ids", "update_pre_rope", "value_cache", "video_end",
    "watch_question", "watched_queries",
]


def test_class_surface_is_unchanged():
    import retake.longvideo_cache as lc

    assert sorted(n for n in dir(lc.PivotKVCache) if n not in dir(lc.DynamicCache)) == SURFACE
    assert isinstance(lc.PivotKVCache.video_end, property)


def test_module_exports_are_unchanged():
    import retake.longvideo_cache as lc

    assert lc.__all__ == ["repeat_kv", "rotate_half", "apply_multimodal_rotary_pos_emb", "apply_rotary_pos_emb",
                          "PivotKVCache", "CacheMark", "build_kvcache", "DynamicCache"]


@pytest.mark.parametrize("name", ["mark", "rewind", "crop", "fork", "update_pre_rope", "append_pre_rope", "after_forward"])
def test_user_facing_methods_keep_their_docstrings(name):
    import retake.longvideo_cache as lc

    doc = getattr(lc.PivotKVCache, name).__doc__
    assert doc and doc.strip()
