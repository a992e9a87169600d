#!/usr/bin/env python
"""What reading an annotation costs (sbgpu_gtf_*): a generated GTF at annotation scale -- 60 000 genes with C3's
isoform law (1 + Geom(0.25), at most 200), about ten exons a transcript, gene / transcript / exon / CDS lines and attribute text
as long as a public annotation's -- read by the device form stage by stage, and by the host form on one thread beside it.

  python tools/bench_gtf.py --out profiles/gtf_bench.json

  upload_ms            the file's bytes host -> device (a torch copy of a pageable array, device events around it)
  device_call_ms       sbgpu_gtf_read_device on bytes that are in HBM, host clock around the call (it synchronises): `reps` calls
                       after a warm-up, median with min - max
  stage_ms             with sbgpu_set_timing on, the call's launches as stages of their own: gtf_line_index, gtf_parse, gtf_sorts
                       (compact, the two radix sorts, the heads and their scan), gtf_merge (the pass per transcript and the scan
                       of the names' sizes), gtf_names_copy_back (the gather and the device -> host copies)
  host_structure_ms    device_call_ms minus the stages: the order, the loci, the arrays, the segments (and the call's waits)
  host_form_ms         sbgpu_gtf_read_host, one thread
It records and gates nothing."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def generate(n_genes, seed=0x6774):
    rng = np.random.Generator(np.random.PCG64(seed))
    niso = np.minimum(rng.geometric(0.25, n_genes), 200)
    out, pos = ["##description: generated annotation", "##provider: tools/bench_gtf.py"], 10000
    for g in range(n_genes):
        chrom, strand = "chr%d" % (1 + g * 24 // n_genes), "+-"[g & 1]
        if g and chrom != "chr%d" % (1 + (g - 1) * 24 // n_genes):
            pos = 10000   # (a chromosome's coordinates begin again)
        gid, gname = "ENSG%011d.%d" % (g, 1 + g % 17), "GENE%d" % g
        n_pool = int(rng.integers(8, 20))
        lens, gaps = rng.integers(40, 600, n_pool), rng.integers(80, 5000, n_pool)
        left = pos + np.concatenate([[0], np.cumsum(lens + gaps)[:-1]])
        right = left + lens - 1
        pos = int(right[-1]) + int(rng.integers(500, 20000))
        gattr = 'gene_id "%s"; gene_type "protein_coding"; gene_name "%s"; level 2; hgnc_id "HGNC:%d"; havana_gene "OTTHUMG%011d.2";' % (gid, gname, g, g)
        out.append("%s\tHAVANA\tgene\t%d\t%d\t.\t%s\t.\t%s" % (chrom, left[0], right[-1], strand, gattr))
        for t in range(int(niso[g])):
            tid = "ENST%011d.%d" % (g * 200 + t, 1 + t % 9)
            k = min(n_pool, max(1, int(rng.normal(10, 3))))
            pick = np.sort(rng.choice(n_pool, k, replace=False))
            tattr = ('gene_id "%s"; transcript_id "%s"; gene_type "protein_coding"; gene_name "%s"; transcript_type "protein_coding"; '
                     'transcript_name "%s-2%02d"; level 2; protein_id "ENSP%011d.3"; transcript_support_level "1"; hgnc_id "HGNC:%d"; '
                     'tag "basic"; tag "Ensembl_canonical"; tag "CCDS"; havana_gene "OTTHUMG%011d.2"; havana_transcript "OTTHUMT%011d.1";'
                     % (gid, tid, gname, gname, t, g * 200 + t, g, g, g * 200 + t))
            out.append("%s\tHAVANA\ttranscript\t%d\t%d\t.\t%s\t.\t%s" % (chrom, left[pick[0]], right[pick[-1]], strand, tattr))
            for n, e in enumerate(pick):
                xattr = tattr[:tattr.index("level 2;")] + 'exon_number %d; exon_id "ENSE%011d.1"; ' % (n + 1, g * 32 + int(e)) + tattr[tattr.index("level 2;"):]
                out.append("%s\tHAVANA\texon\t%d\t%d\t.\t%s\t.\t%s" % (chrom, left[e], right[e], strand, xattr))
                if 0 < n < k - 1:
                    out.append("%s\tHAVANA\tCDS\t%d\t%d\t.\t%s\t%d\t%s" % (chrom, left[e], right[e], strand, n % 3, xattr))
    return ("\n".join(out) + "\n").encode()


def stats(ms):
    return {"median": float(np.median(ms)), "min": float(min(ms)), "max": float(max(ms))}


def stages(ctx):
    ms, names = (C.c_float * 16)(), (C.c_char_p * 16)()
    n = ctx.L.sbgpu_last_stage_ms(ctx.h, 16, ms, names)
    return {names[i].decode(): float(ms[i]) for i in range(max(n, 0))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genes", type=int, default=60000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gtf_bench.json"))
    args = ap.parse_args()
    import torch
    from strawberry_amd import _lib, em, gtf
    ctx = em.default_context(0)
    L, dev = ctx.L, torch.device("cuda", ctx.device)
    t0 = time.perf_counter()
    data = generate(args.genes)
    doc = {"tool": "tools/bench_gtf.py", "build_id": L.sbgpu_build_id().decode(), "device": torch.cuda.get_device_name(dev), "reps": args.reps,
           "genes": args.genes, "file_bytes": len(data), "generate_s": time.perf_counter() - t0, "limits": gtf.limits()}
    host_arr = np.frombuffer(data, np.uint8).copy()
    t = time.perf_counter()
    g_host = gtf.read_gtf(host_arr)
    doc["host_form_first_ms"] = (time.perf_counter() - t) * 1e3
    doc["info"] = g_host.info
    h, opts = C.c_void_p(), _lib.sbgpu_gtf_opts_t()
    host_ms = []
    for _ in range(max(1, args.reps // 4)):
        t = time.perf_counter()
        _lib.check(L.sbgpu_gtf_read_host(host_arr.ctypes.data, host_arr.size, C.byref(opts), C.byref(h)), "sbgpu_gtf_read_host")
        host_ms.append((time.perf_counter() - t) * 1e3)
        L.sbgpu_gtf_destroy(h)
    doc["host_form_ms"] = stats(host_ms)
    up = []
    for _ in range(args.reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        d = torch.from_numpy(host_arr).to(dev)
        e1.record()
        torch.cuda.synchronize(dev)
        up.append(e0.elapsed_time(e1))
    doc["upload_ms"] = stats(up[1:])

    def call():
        t = time.perf_counter()
        _lib.check(L.sbgpu_gtf_read_device(ctx.h, d.data_ptr(), int(d.numel()), C.byref(opts), None, C.byref(h)), "sbgpu_gtf_read_device")
        ms = (time.perf_counter() - t) * 1e3
        L.sbgpu_gtf_destroy(h)
        return ms
    # the results first: the device form's are the host form's
    g_dev = gtf.read_gtf(d, ctx=ctx)
    for name in ("iso_off", "exon_off", "exon_left", "exon_right", "seg_off", "seg_left", "seg_right", "cluster_ref", "cluster_left", "cluster_right",
                 "cluster_strand", "iso_len", "iso_strand", "line_status"):
        assert np.array_equal(getattr(g_dev, name), getattr(g_host, name)), name
    for name in ("gene_id", "gene_name", "transcript_id", "chrom", "info"):
        assert getattr(g_dev, name) == getattr(g_host, name), name
    doc["device_equals_host"] = True
    del g_dev
    call()
    doc["device_call_ms"] = stats([call() for _ in range(args.reps)])
    _lib.check(L.sbgpu_set_timing(ctx.h, 1), "sbgpu_set_timing")
    try:
        per, walls = {}, []
        for _ in range(args.reps):
            walls.append(call())
            for k, v in stages(ctx).items():
                per.setdefault(k, []).append(v)
    finally:
        L.sbgpu_set_timing(ctx.h, 0)
    doc["stage_ms"] = {k: stats(v) for k, v in per.items()}
    doc["timed_call_ms"] = stats(walls)
    doc["host_structure_ms"] = float(np.median(walls)) - sum(float(np.median(v)) for v in per.values())
    doc["bytes_per_s_device_call"] = len(data) / (doc["device_call_ms"]["median"] * 1e-3)
    doc["bytes_per_s_host_form"] = len(data) / (doc["host_form_ms"]["median"] * 1e-3)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps({k: doc[k] for k in ("file_bytes", "info", "upload_ms", "device_call_ms", "stage_ms", "host_structure_ms", "host_form_ms")}))


if __name__ == "__main__":
    main()
