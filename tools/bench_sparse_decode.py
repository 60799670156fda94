#!/usr/bin/env python
"""The page-sparse decode (retake/_sparse_decode.py, rtk_attention_decode_sparse) at the headline geometry, beside what it
has to be weighed against - all in ONE process, HIP events, the samples of every measurement INTERLEAVED (so that all see
the same drift of clocks and the same neighbours), medians of `reps` with quartiles.

    python tools/bench_sparse_decode.py [--out profiles/sparse_decode_bench.json] [--reps 15] [--warmup 3] [--parent-lib PATH]..

28 layers, Hq 28 / Hkv 4 / D 128, bf16, n = 100 352 region rows per layer behind 37 pinned rows, 64 tail rows; one layer's
call, one query row per head; keep_rows 4 096 / 8 192 / 16 384:
  decode_full        rtk_attention_decode over ALL rows of the layer: the call the sparse chain replaces.  With
                     --parent-lib it is taken from that library (the parent commit's build), else from this build's
                     (tools/kernel_diff.py: the kernel compiles to the same code).  --parent-lib also adds the rows
                     sparse_K@parent1 and paged_K@parent1 (--fp8: sparse8_K, paged8_K and theirs), measured from that library
                     in the same interleaving, and `versus_parent`; given twice - a copy of the library under another file
                     name is @parent2 - the parent against its copy is the job's noise;
  sparse_K           the whole chain, rtk_attention_decode_sparse: bound, selection, paged attention, combine;
  bound              its first launch alone (rtk_attention_page_bound over the layer's 3 136 pages);
  select_K           its second (rtk_pivotkv_budget_select_batched, one unit per kv head);
  paged_K            its third and fourth (rtk_attention_decode_paged with the chain's lists: paged kernel + combine);
  focused_K          the packed call over a focused cache of the same keep_rows (PivotKVCache.focus): pinned + K + tail rows;
  summary_build      rtk_pivotkv_page_summary_batched over the 28 layers: what arming costs;
  copy_k_bytes       rtk_profile_copy of the K bytes the summary build reads (what a plain copy of them costs).
One JSON document; a summary on stdout.  Needs the GPU: there is no other way to get a time.

    python tools/bench_sparse_decode.py --fp8 [--out profiles/sparse_decode_fp8_bench.json] [--parent-lib PATH]

The same over an fp8 archive (sparse_decode(cache, archive=True), rtk_attention_decode_sparse_fp8kv): 28 layers x 100 352
archive rows, 37 pinned + 64 tail 16-bit rows, the buffers filled directly (layer 0: quantised random rows; the other layers,
which only the summary build reads: random finite codes):
  fp8_full           (a) rtk_attention_decode_fp8kv over the full archive (from --parent-lib when given): the call the chain replaces;
  sparse8_K          the whole chain, rtk_attention_decode_sparse_fp8kv;
  gathered8_K        (b) rtk_attention_decode_fp8kv over a gathered archive of K rows: what a focused fp8 cache pays per token;
  sparse16_K         (c) the 16-bit chain, rtk_attention_decode_sparse, on the dequantised rows;
  summary_build8     rtk_pivotkv_page_summary_fp8k_batched over the 28 layers: what arming costs;
  copy_k_code_bytes  rtk_profile_copy of the K codes' bytes.

    python tools/bench_sparse_decode.py --wide [--out profiles/sparse_decode_wide_bench.json] [--parent-lib PATH]

Several new tokens (sparse_decode(cache, wide=True), rtk_attention_decode_sparse_wide): one layer of the same geometry, its
buffers filled directly, Lq 3 / 6 / 9 query rows (21 / 42 / 63 packed rows) x keep_rows 4 096 / 8 192 / 16 384; then one row
each at Hq 8 / Hkv 4 (Lq 9) and Hq 8 / Hkv 8 (Lq 17) with keep_rows 8 192, their names prefixed g2_ / g1_:
  wide_full_L        (a) rtk_attention_decode_wide over ALL rows (from --parent-lib when given): what multi_token_attention pays;
  chunk_L            (b) the chunk kernel over all rows (chunk_attention as it is): what a cache without that key pays;
  sparse_wide_L_K    (c) the whole chain, rtk_attention_decode_sparse_wide: bound, selection, wide paged attention, combine;
  bound_L, select_K, paged_wide_L_K   its launches alone, on the chain's own operands;
  sparse_1_K         (d) the narrow chain, rtk_attention_decode_sparse, one query row on the same buffers.
A gain over (a) is claimed (`beats_wide_full`) only where the difference of medians exceeds the sum of the two interquartile
ranges."""
from __future__ import annotations

import argparse
import ctypes as C
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "video-retake_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch  # noqa: E402

import retake._native as nv  # noqa: E402
import retake._sparse_decode as sd  # noqa: E402
from bench_focus import D, Hkv, Hq, KEEPS, LAYERS, N, PINNED, QUESTION, arm, parent, stat  # noqa: E402
from retake.native_attention import chunk_attention  # noqa: E402

PAGES = N // 32
KEEP_PAGES = {K: min(-(-K // 32), PAGES) for K in KEEPS}
BF = nv.RTK_BF16
_HOLD = []   # the workspaces of `sized`: alive as long as the process
of = lambda chain, row: [(r, fn) for r, fn in chain.items() if r.split("@")[0] == row]   # noqa: E731  (a row of every library)


def libraries(args):
    """[(tag, library)]: this build's under "", then every --parent-lib under "@parent1", "@parent2", .. with `names` bound."""
    names = ["rtk_attention_decode", "rtk_attention_decode_workspace_bytes", "rtk_attention_decode_fp8kv",
             "rtk_attention_decode_workspace_bytes_fp8kv", "rtk_attention_decode_wide", "rtk_attention_decode_wide_workspace_bytes"]
    names += [f"rtk_attention_decode_{c}{k}{w}" for c in ("paged", "sparse") for k in ("", "_fp8kv") for w in ("", "_workspace_bytes")]
    libs = [("", nv.lib)]
    for i, path in enumerate(args.parent_lib):
        lib = C.CDLL(path)
        for name in names:
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = nv._SIGNATURES[name]
        libs.append((f"@parent{i + 1}", lib))
    return libs


def call(lib, name, *a):
    """fn(): one checked call of the library's entry point"""
    fn = getattr(lib, name)
    return lambda: nv.check(fn(*a), name)


def sized(lib, query, *shape):
    """(pointer, bytes) of a fresh workspace of the size the library's query states"""
    need = getattr(lib, query)(*shape)
    _HOLD.append(torch.empty(need, dtype=torch.uint8, device="cuda:0"))
    return nv.ptr(_HOLD[-1]), need


def chain_rows(libs, kind, Lk, region, call_args, picks, stream):
    """{row: fn} of rtk_attention_decode_{paged,sparse}{kind} from every library: rows paged_K / sparse_K (fp8: paged8_K /
    sparse8_K) + the library's tag.  `region`: of the queries, between Lk and keep_pages; picks[chain](K): the list or summ + stride."""
    rows = {}
    for tag, lib in libs:
        for K in KEEPS:
            for chain, pick in picks.items():
                name = f"rtk_attention_decode_{chain}{kind}"
                ws = sized(lib, name + "_workspace_bytes", Hq, Hkv, 1, Lk, *region, KEEP_PAGES[K], D, BF)
                rows[f"{chain}{'8' if kind else ''}_{K}{tag}"] = call(lib, name, *call_args, *pick(K), KEEP_PAGES[K], *ws, stream)
    return rows


def select_lists(q1, summ, stream):
    """(bound, {K: select}, {K: lists}): the chain's first two launches on its own operands, run once"""
    ub = torch.empty((Hkv, PAGES), dtype=torch.float32, device=q1.device)
    bound = call(nv.lib, "rtk_attention_page_bound", nv.ptr(q1), q1.stride(1), q1.stride(2), nv.ptr(summ), summ.stride(0), Hq, Hkv, 1,
                 PAGES, D, BF, nv.ptr(ub), stream)
    bound()
    lists = {K: torch.empty((Hkv, KEEP_PAGES[K]), dtype=torch.int32, device=q1.device) for K in KEEPS}
    select = {}
    for K in KEEPS:
        units = (nv.BudgetSelectUnit * Hkv)(*[nv.BudgetSelectUnit(ub[h].data_ptr(), lists[K][h].data_ptr(), PAGES, KEEP_PAGES[K])
                                              for h in range(Hkv)])
        select[K] = call(nv.lib, "rtk_pivotkv_budget_select_batched", units, Hkv, stream)
        select[K]()
    return bound, select, lists


def measure_and_report(args, work, report, method, derive, what="one layer's call, one query row per head"):
    """Every row of `work` [(name, fn)] INTERLEAVED, HIP events, the libraries of a row taking turns at going first; `report`
    gains each row's statistics, what `derive` adds (it returns the mode's lines for stdout) and, with --parent-lib, the
    samples of the contested rows and `versus_parent`."""
    samples = {name: [] for name, _ in work}
    groups = [list(rows) for _, rows in itertools.groupby(work, lambda row: row[0].split("@")[0])]   # a row of every library
    for rep in range(args.warmup + args.reps):
        for name, fn in (row for rows in groups for row in rows[rep % len(rows):] + rows[:rep % len(rows)]):   # interleaved
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if rep >= args.warmup:
                samples[name].append(e0.elapsed_time(e1) * 1e3)
    report["method"] = (f"one process, HIP events, interleaved, median and quartiles of {args.reps} after {args.warmup} warm-up "
                        f"rounds; {what}" + method)
    for name in samples:
        report[name] = stat(samples[name])
    lines = derive(report)
    rows = [name for name in samples if name + "@parent1" in samples]
    if rows:
        for name in samples:
            if name.split("@")[0] in rows:
                report[name]["samples_us"] = [round(x, 1) for x in samples[name]]
        gap = lambda a, b: {n: round(report[n + a]["median_us"] - report[n + b]["median_us"], 1) for n in rows}   # noqa: E731
        vs = report["versus_parent"] = {"new_minus_parent_us": gap("", "@parent1")}
        if len(args.parent_lib) > 1:
            vs["parent_copy_minus_parent_us"] = gap("@parent2", "@parent1")
            vs["noise_us"] = max(abs(d) for d in vs["parent_copy_minus_parent_us"].values())
            vs["within_noise"] = {n: abs(d) <= vs["noise_us"] for n, d in vs["new_minus_parent_us"].items()}
        lines.append("new - parent, us: " + ", ".join(f"{n} {d:+.1f}" for n, d in vs["new_minus_parent_us"].items())
                     + (f"; noise (the parent's copy - the parent) {vs['noise_us']:.1f}" if "noise_us" in vs else ""))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")
    for name in samples:
        print(f"{name}: {report[name]['median_us']:.0f} us (quartiles {report[name]['q1_us']:.0f} .. {report[name]['q3_us']:.0f})")
    print("\n".join(lines + ["wrote " + args.out]))


def main_fp8(args, libs, full_lib):
    from retake.native_attention import fp8_dequantize_rows, fp8_quantize_rows

    dev, stream = torch.device("cuda:0"), nv.stream()
    g = torch.Generator(device=dev).manual_seed(7)
    Lk = PINNED + QUESTION   # the 16-bit rows: pinned, then everything behind the video
    bf, scale = torch.bfloat16, D ** -0.5
    rnd = lambda *shape: (1.7 * torch.randn(shape, generator=g, device=dev)).to(bf)   # noqa: E731
    q1, k16, v16 = rnd(1, Hq, 1, D), rnd(1, Hkv, Lk, D), rnd(1, Hkv, Lk, D)
    k8, ks = fp8_quantize_rows(rnd(1, Hkv, N, D))
    v8, vs = fp8_quantize_rows(rnd(1, Hkv, N, D))
    out = torch.empty((1, 1, Hq, D), dtype=bf, device=dev)
    q3 = (nv.ptr(q1), q1.stride(1), q1.stride(2))

    def fp8kv_args(k8, v8, ks, vs):
        return q3 + (nv.ptr(k16), nv.ptr(v16), k16.stride(1), k16.stride(2), nv.ptr(k8), nv.ptr(v8), nv.ptr(ks), nv.ptr(vs),
                     k8.shape[2], k8.stride(1), ks.stride(1), nv.ptr(out), Hq, Hkv, 1, Lk, Lk - 1, D, BF, scale)

    # ---- (a) the call the chain replaces: from the parent commit's library when given -----------------------------------
    full_args = fp8kv_args(k8, v8, ks, vs)
    run_full = call(full_lib, "rtk_attention_decode_fp8kv", *full_args,
                    *sized(full_lib, "rtk_attention_decode_workspace_bytes_fp8kv", Hq, Hkv, 1, Lk, N, D, BF), stream)

    # ---- the index over the K codes of every layer, and a plain copy of those bytes --------------------------------------
    codes = [k8] + [(torch.randint(0, 127, (1, Hkv, N, D), generator=g, device=dev, dtype=torch.uint8)
                     | (torch.randint(0, 2, (1, Hkv, N, D), generator=g, device=dev, dtype=torch.uint8) << 7)) for _ in range(LAYERS - 1)]
    scales = [ks] + [torch.full((1, Hkv, N), 2.0 ** -6, dtype=torch.float32, device=dev) for _ in range(LAYERS - 1)]
    summs = [torch.empty((Hkv, PAGES, 2, D), dtype=bf, device=dev) for _ in range(LAYERS)]
    units = (nv.PageSummaryFp8kUnit * LAYERS)()
    for u, c8, s8, sm in zip(units, codes, scales, summs):
        u.k8, u.k8_stride_h, u.k_scale, u.scale_stride_h, u.n = c8.data_ptr(), c8.stride(1), s8.data_ptr(), s8.stride(1), N
        u.summ, u.summ_stride_h = sm.data_ptr(), sm.stride(0)
    run_summary = call(nv.lib, "rtk_pivotkv_page_summary_fp8k_batched", units, LAYERS, Hkv, D, BF, stream)
    run_summary()
    summ = summs[0]
    code_bytes = LAYERS * Hkv * N * D
    csrc, cdst = torch.zeros(code_bytes, dtype=torch.uint8, device=dev), torch.empty(code_bytes, dtype=torch.uint8, device=dev)
    run_copy = call(nv.lib, "rtk_profile_copy", nv.ptr(cdst), nv.ptr(csrc), code_bytes, stream)

    # ---- the chain; with --parent-lib from every library, and its third and fourth launches (paged8_K) on its own lists ----
    picks = {"sparse": lambda K: (nv.ptr(summ), summ.stride(0))}
    if args.parent_lib:
        lists = select_lists(q1, summ, stream)[2]
        picks["paged"] = lambda K: (nv.ptr(lists[K]),)
    chain = chain_rows(libs, "_fp8kv", Lk, (N,), full_args, picks, stream)

    # ---- (b) the packed fp8 call over a gathered archive of keep_rows rows ------------------------------------------------
    gathered, run_gathered8 = [], {}
    for K in KEEPS:
        idx = torch.randperm(N, generator=g, device=dev)[:K].sort().values
        gathered.append(tuple(t.index_select(2, idx).contiguous() for t in (k8, v8, ks, vs)))   # (kept alive beside their pointers)
        run_gathered8[K] = call(nv.lib, "rtk_attention_decode_fp8kv", *fp8kv_args(*gathered[-1]),
                                *sized(nv.lib, "rtk_attention_decode_workspace_bytes_fp8kv", Hq, Hkv, 1, Lk, K, D, BF), stream)

    # ---- (c) the 16-bit chain on the dequantised rows: [pinned | dequantised archive | tail] in one buffer -----------------
    ve, L16 = PINNED + N, PINNED + N + QUESTION
    kd = torch.cat([k16[:, :, :PINNED], fp8_dequantize_rows(k8, ks, bf), k16[:, :, PINNED:]], dim=2).contiguous()
    vd = torch.cat([v16[:, :, :PINNED], fp8_dequantize_rows(v8, vs, bf), v16[:, :, PINNED:]], dim=2).contiguous()
    summ16 = torch.empty((Hkv, PAGES, 2, D), dtype=bf, device=dev)
    u16 = (nv.PageSummaryUnit * 1)()
    u16[0].k, u16[0].k_stride_h, u16[0].first, u16[0].n = kd.data_ptr(), kd.stride(1), PINNED, N
    u16[0].summ, u16[0].summ_stride_h = summ16.data_ptr(), summ16.stride(0)
    call(nv.lib, "rtk_pivotkv_page_summary_batched", u16, 1, Hkv, D, BF, stream)()
    args16 = q3 + (nv.ptr(kd), nv.ptr(vd), kd.stride(1), kd.stride(2), nv.ptr(out), Hq, Hkv, 1, L16, L16 - 1, D, BF, scale, PINNED, ve)
    sparse16 = chain_rows(libs[:1], "", L16, (PINNED, ve), args16, {"sparse": lambda K: (nv.ptr(summ16), summ16.stride(0))}, stream)

    work = [("fp8_full", run_full), ("summary_build8", run_summary), ("copy_k_code_bytes", run_copy)]
    for K in KEEPS:
        work += of(chain, f"sparse8_{K}") + [(f"gathered8_{K}", run_gathered8[K]), (f"sparse16_{K}", sparse16[f"sparse_{K}"])]
        work += of(chain, f"paged8_{K}")

    report = {"device": torch.cuda.get_device_name(0),
              "geometry": {"layers": LAYERS, "Hq": Hq, "Hkv": Hkv, "D": D, "dtype": "bf16", "archive_rows": N, "pages": PAGES,
                           "pinned": PINNED, "tail": QUESTION, "keep_rows": list(KEEPS), "k_code_bytes": code_bytes,
                           "summary_bytes": LAYERS * Hkv * PAGES * 2 * D * 2},
              "fp8_full_from": "parent commit's library" if args.parent_lib else "this build (same kernel code as the parent's)"}

    def derive(report):
        iqr = lambda r: r["q3_us"] - r["q1_us"]   # noqa: E731
        lines = []
        for K in KEEPS:
            r, full = report[f"sparse8_{K}"], report["fp8_full"]
            r.update(full_over_sparse=round(full["median_us"] / r["median_us"], 2),
                     sparse_over_gathered=round(r["median_us"] / report[f"gathered8_{K}"]["median_us"], 2),
                     sparse_over_16bit_chain=round(r["median_us"] / report[f"sparse16_{K}"]["median_us"], 2),
                     beats_full_by_more_than_both_iqrs=bool(full["median_us"] - r["median_us"] > max(iqr(full), iqr(r))))
            lines.append(f"keep_rows {K}: the full fp8 call {r['full_over_sparse']:.2f} x the chain; the chain "
                         f"{r['sparse_over_gathered']:.2f} x the call over a gathered archive, {r['sparse_over_16bit_chain']:.2f} x the "
                         "16-bit chain")
        report["summary_build8"]["time_over_copy"] = round(report["summary_build8"]["median_us"] / report["copy_k_code_bytes"]["median_us"], 3)
        return lines + [f"summary build {report['summary_build8']['time_over_copy']:.2f} x the plain copy of the K codes' bytes"]

    measure_and_report(args, work, report, "", derive)


def main_wide(args, full_lib):
    dev, stream = torch.device("cuda:0"), nv.stream()
    g = torch.Generator(device=dev).manual_seed(7)
    bf, scale = torch.bfloat16, D ** -0.5
    ve, Lk = PINNED + N, PINNED + N + QUESTION
    rnd = lambda *shape: (1.7 * torch.randn(shape, generator=g, device=dev)).to(bf)   # noqa: E731
    work, routes, hold = [], {}, []

    def geometry(prefix, hq, hkv, Lqs, keeps, narrow):
        """The rows of one head geometry over a layer of its own: [(name, fn)] appended to `work`."""
        k, v = rnd(1, hkv, Lk, D), rnd(1, hkv, Lk, D)
        summ = torch.empty((hkv, PAGES, 2, D), dtype=bf, device=dev)
        u = (nv.PageSummaryUnit * 1)()
        u[0].k, u[0].k_stride_h, u[0].first, u[0].n, u[0].summ, u[0].summ_stride_h = k.data_ptr(), k.stride(1), PINNED, N, summ.data_ptr(), summ.stride(0)
        call(nv.lib, "rtk_pivotkv_page_summary_batched", u, 1, hkv, D, BF, stream)()
        ub = torch.empty((hkv, PAGES), dtype=torch.float32, device=dev)
        hold.extend([k, v, summ, ub, u])
        selects = {}
        for Lq in Lqs:
            q = rnd(1, hq, Lq, D)
            out = torch.empty((1, Lq, hq, D), dtype=bf, device=dev)
            hold.extend([q, out])
            a = (nv.ptr(q), q.stride(1), q.stride(2), nv.ptr(k), nv.ptr(v), k.stride(1), k.stride(2), nv.ptr(out), hq, hkv, Lq, Lk,
                 Lk - Lq, D, BF, scale)
            assert (hq // hkv) * Lq > 16
            work.append((f"{prefix}wide_full_{Lq}", call(full_lib, "rtk_attention_decode_wide", *a, *sized(
                full_lib, "rtk_attention_decode_wide_workspace_bytes", hq, hkv, Lq, Lk, D, BF), stream)))
            fws, route = {}, []
            run_chunk = lambda q=q, fws=fws, route=route: chunk_attention(q, k, v, workspace=fws, route=route)   # noqa: E731
            assert run_chunk() is not None
            routes[f"{prefix}chunk_{Lq}"] = route[0]
            work.append((f"{prefix}chunk_{Lq}", run_chunk))
            bound = call(nv.lib, "rtk_attention_page_bound", nv.ptr(q), q.stride(1), q.stride(2), nv.ptr(summ), summ.stride(0), hq,
                         hkv, Lq, PAGES, D, BF, nv.ptr(ub), stream)
            bound()
            work.append((f"{prefix}bound_{Lq}", bound))
            for K in keeps:
                kp = KEEP_PAGES[K]
                chain = "rtk_attention_decode_sparse_wide"
                work.append((f"{prefix}sparse_wide_{Lq}_{K}", call(nv.lib, chain, *a, PINNED, ve, nv.ptr(summ), summ.stride(0), kp, *sized(
                    nv.lib, chain + "_workspace_bytes", hq, hkv, Lq, Lk, PINNED, ve, kp, D, BF), stream)))
                lists = torch.empty((hkv, kp), dtype=torch.int32, device=dev)
                units = (nv.BudgetSelectUnit * hkv)(*[nv.BudgetSelectUnit(ub[h].data_ptr(), lists[h].data_ptr(), PAGES, kp)
                                                      for h in range(hkv)])
                select = call(nv.lib, "rtk_pivotkv_budget_select_batched", units, hkv, stream)
                select()   # (the lists of the last Lq's bounds: the paged launch alone reads them)
                hold.extend([lists, units])
                if K not in selects:
                    selects[K] = select
                    work.append((f"{prefix}select_{K}", select))
                work.append((f"{prefix}paged_wide_{Lq}_{K}", call(nv.lib, "rtk_attention_decode_paged_wide", *a, PINNED, ve, nv.ptr(lists),
                                                                   kp, *sized(nv.lib, "rtk_attention_decode_paged_wide_workspace_bytes", hq,
                                                                              hkv, Lq, Lk, PINNED, ve, kp, D, BF), stream)))
        if narrow:   # (d) one query row on the same buffers
            narrow_rows(prefix, hq, hkv, k, v, summ, keeps)

    def narrow_rows(prefix, hq, hkv, k, v, summ, keeps):
        Lq = 1
        q = rnd(1, hq, Lq, D)
        out = torch.empty((1, Lq, hq, D), dtype=bf, device=dev)
        hold.extend([q, out])
        a = (nv.ptr(q), q.stride(1), q.stride(2), nv.ptr(k), nv.ptr(v), k.stride(1), k.stride(2), nv.ptr(out), hq, hkv, Lq, Lk, Lk - Lq,
             D, BF, scale)
        for K in keeps:
            work.append((f"{prefix}sparse_1_{K}", call(nv.lib, "rtk_attention_decode_sparse", *a, PINNED, ve, nv.ptr(summ), summ.stride(0),
                                                       KEEP_PAGES[K], *sized(nv.lib, "rtk_attention_decode_sparse_workspace_bytes", hq, hkv,
                                                                             Lq, Lk, PINNED, ve, KEEP_PAGES[K], D, BF), stream)))

    LQS = (3, 6, 9)
    geometry("", Hq, Hkv, LQS, KEEPS, True)
    geometry("g2_", 8, 4, (9,), (8192,), False)
    geometry("g1_", 8, 8, (17,), (8192,), False)

    report = {"device": torch.cuda.get_device_name(0),
              "geometry": {"layers": LAYERS, "Hq": Hq, "Hkv": Hkv, "D": D, "dtype": "bf16", "n": N, "pages": PAGES, "pinned": PINNED,
                           "tail": QUESTION, "keep_rows": list(KEEPS), "Lq": list(LQS),
                           "g2_": {"Hq": 8, "Hkv": 4, "Lq": 9, "keep_rows": 8192}, "g1_": {"Hq": 8, "Hkv": 8, "Lq": 17, "keep_rows": 8192}},
              "wide_full_from": "parent commit's library" if args.parent_lib else "this build (same kernel code as the parent's)",
              "chunk_routes": routes}

    def derive(report):
        iqr = lambda r: r["q3_us"] - r["q1_us"]   # noqa: E731
        lines = []
        for prefix, Lqs, keeps in (("", LQS, KEEPS), ("g2_", (9,), (8192,)), ("g1_", (17,), (8192,))):
            for Lq in Lqs:
                full, chunk = report[f"{prefix}wide_full_{Lq}"], report[f"{prefix}chunk_{Lq}"]
                for K in keeps:
                    r = report[f"{prefix}sparse_wide_{Lq}_{K}"]
                    r.update(wide_full_over_chain=round(full["median_us"] / r["median_us"], 2),
                             chunk_over_chain=round(chunk["median_us"] / r["median_us"], 2),
                             beats_wide_full=bool(full["median_us"] - r["median_us"] > iqr(full) + iqr(r)))
                    lines.append(f"{prefix}Lq {Lq} keep_rows {K}: the chain {r['median_us']:.0f} us; the wide call over all rows "
                                 f"{r['wide_full_over_chain']:.2f} x, the chunk kernel {r['chunk_over_chain']:.2f} x; gain over the wide "
                                 f"call beyond both IQRs: {r['beats_wide_full']}")
        return lines

    measure_and_report(args, work, report, "; the launches alone run on the chain's own operands", derive,
                       "one layer's call, Lq query rows per head")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="default: profiles/sparse_decode_bench.json (--fp8: sparse_decode_fp8_bench.json, "
                    "--wide: sparse_decode_wide_bench.json)")
    ap.add_argument("--fp8", action="store_true", help="the chain over an fp8 archive (rtk_attention_decode_sparse_fp8kv)")
    ap.add_argument("--wide", action="store_true", help="several new tokens (rtk_attention_decode_sparse_wide)")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parent-lib", action="append", default=[], metavar="PATH",
                    help="libretake_hip.so of the parent commit (see above); a second one, a copy under another name, is @parent2")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sparse_decode.py measures on the GPU; none is visible (Time: not measured)")
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "sparse_decode_fp8_bench.json" if args.fp8 else
                                "sparse_decode_wide_bench.json" if args.wide else "sparse_decode_bench.json")
    libs = libraries(args)
    full_lib = libs[1 if args.parent_lib else 0][1]
    if args.fp8:
        return main_fp8(args, libs, full_lib)
    if args.wide:
        return main_wide(args, full_lib)
    dev, stream = torch.device("cuda:0"), nv.stream()
    g = torch.Generator(device=dev).manual_seed(7)
    cache = parent(dev, g)
    st = cache._layers[0]
    ve, Lk = PINNED + N, PINNED + N + QUESTION
    q1 = (1.7 * torch.randn((1, Hq, 1, D), generator=g, device=dev)).bfloat16()
    k, v = st._k[:, :, :Lk], st._v[:, :, :Lk]
    out = torch.empty((1, 1, Hq, D), dtype=torch.bfloat16, device=dev)
    call_args = (nv.ptr(q1), q1.stride(1), q1.stride(2), nv.ptr(k), nv.ptr(v), k.stride(1), k.stride(2), nv.ptr(out), Hq, Hkv, 1, Lk,
                 Lk - 1, D, BF, D ** -0.5)

    # ---- the call the chain replaces: from the parent commit's library when given --------------------------------------
    run_full = call(full_lib, "rtk_attention_decode", *call_args,
                    *sized(full_lib, "rtk_attention_decode_workspace_bytes", Hq, Hkv, 1, Lk, D, BF), stream)

    # ---- the index, the chain and its launches alone (with --parent-lib: paged_K and sparse_K from every library) --------
    sd.sparse_decode(cache, max(KEEPS))
    summs = dict(cache._sparse.summ)   # (kept alive here: dense_decode below frees the cache's references)
    summ = summs[0]
    run_bound, run_select, lists = select_lists(q1, summ, stream)
    chain = chain_rows(libs, "", Lk, (PINNED, ve), call_args + (PINNED, ve),
                       {"sparse": lambda K: (nv.ptr(summ), summ.stride(0)), "paged": lambda K: (nv.ptr(lists[K]),)}, stream)

    # ---- the summary build and a plain copy of the K bytes it reads -----------------------------------------------------
    units = (nv.PageSummaryUnit * LAYERS)()
    for l, (u, s) in enumerate(zip(units, cache._layers)):
        sm = summs[l]
        u.k, u.k_stride_h, u.first, u.n, u.summ, u.summ_stride_h = s._k.data_ptr(), s._k.stride(1), PINNED, N, sm.data_ptr(), sm.stride(0)
    run_summary = call(nv.lib, "rtk_pivotkv_page_summary_batched", units, LAYERS, Hkv, D, BF, stream)
    k_bytes = LAYERS * Hkv * N * D * 2
    csrc, cdst = torch.zeros(k_bytes, dtype=torch.uint8, device=dev), torch.empty(k_bytes, dtype=torch.uint8, device=dev)
    run_copy = call(nv.lib, "rtk_profile_copy", nv.ptr(cdst), nv.ptr(csrc), k_bytes, stream)

    # ---- the packed call over a focused cache of the same keep_rows -----------------------------------------------------
    queries = [(1.7 * torch.randn((Hq, 64, D), generator=g, device=dev)).bfloat16() for _ in range(LAYERS)]
    sd.dense_decode(cache)
    arm(cache, 64, queries)
    small, fws, route = {}, {}, []
    for K in KEEPS:
        fc = cache.focus(K)
        s0 = fc._layers[0]
        small[K] = (s0._k[:, :, :s0.length].clone(), s0._v[:, :, :s0.length].clone())   # one layer's rows: the caches are freed
        del fc
    cache.unwatch_question()

    def run_focused(K):
        assert chunk_attention(q1, *small[K], workspace=fws, packed_gqa=True, route=route) is not None

    run_focused(KEEPS[0])
    assert route == ["packed"], route

    work = [("decode_full", run_full), ("bound", run_bound), ("summary_build", run_summary), ("copy_k_bytes", run_copy)]
    for K in KEEPS:
        work += of(chain, f"sparse_{K}") + [(f"select_{K}", run_select[K])] + of(chain, f"paged_{K}")
        work += [(f"focused_{K}", lambda K=K: run_focused(K))]

    report = {"device": torch.cuda.get_device_name(0),
              "geometry": {"layers": LAYERS, "Hq": Hq, "Hkv": Hkv, "D": D, "dtype": "bf16", "n": N, "pages": PAGES, "pinned": PINNED,
                           "tail": QUESTION, "keep_rows": list(KEEPS), "k_bytes": k_bytes,
                           "summary_bytes": LAYERS * Hkv * PAGES * 2 * D * 2},
              "decode_full_from": "parent commit's library" if args.parent_lib else "this build (same kernel code as the parent's)"}

    def derive(report):
        lines = []
        for K in KEEPS:
            r = report[f"sparse_{K}"]
            r.update(full_over_sparse=round(report["decode_full"]["median_us"] / r["median_us"], 2),
                     sparse_over_focused=round(r["median_us"] / report[f"focused_{K}"]["median_us"], 2))
            lines.append(f"keep_rows {K}: the full call {r['full_over_sparse']:.2f} x the sparse chain, the chain "
                         f"{r['sparse_over_focused']:.2f} x the call over a focused cache")
        report["summary_build"]["time_over_copy"] = round(report["summary_build"]["median_us"] / report["copy_k_bytes"]["median_us"], 3)
        return lines + [f"summary build {report['summary_build']['time_over_copy']:.2f} x the plain copy of K's bytes"]

    measure_and_report(args, work, report, "; the launches alone run on the chain's own operands", derive)


if __name__ == "__main__":
    main()
