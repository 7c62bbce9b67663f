#!/usr/bin/env python3
"""Time ramcrc_recovery_append_device against a device-to-device copy of the
same bytes.

    python tools/recovery_append_bench.py [--nseg 512] [--values 64,1024,4096]
                                          [--out profiles/recovery_append]

Sources are RecoverSegmentBenchmark-shaped 8 MiB segments built on the device
(fill_objects), walked once; every record is placed in partition (record index
mod 8).  After warm-up calls, each timed call is bracketed by device events.
The yardstick, in the same process, is a contiguous device-to-device copy of
as many bytes as the call appended (torch's copy_ of uint8 tensors, which
issues hipMemcpyAsync): the floor for reading every byte once and writing it
once.  One JSON file per value size, and one summary line on stdout.

The measurement runs in one child process under a time limit; this process
never opens the GPU.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MiB = 1 << 20


def measure(args):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from ramcloud_amd import build, ramcrc, segments

    build.build()
    if not torch.cuda.is_available():
        raise SystemExit("recovery_append_bench: no GPU (no fallback)")
    ctx = ramcrc.Context(0)
    cap, nseg, n_part = 8 * MiB, args.nseg, 8
    out_stride = cap // n_part + 16 * 1024
    out_capacity = out_stride
    n_out = nseg * n_part
    d = torch.empty(nseg * cap, dtype=torch.uint8, device="cuda")
    d.random_(0, 256)
    out = torch.empty(n_out * out_stride, dtype=torch.uint8, device="cuda")
    certs = torch.zeros((n_out, 2), dtype=torch.int32, device="cuda")
    stat = torch.zeros((n_out, 2), dtype=torch.int32, device="cuda")
    results = []
    for value_len in args.values:
        dc = torch.zeros((nseg, 2), dtype=torch.int32, device="cuda")
        per, seg_len, _ = ctx.fill_objects(d, cap, cap, nseg, value_len, certs=dc)
        ecap = nseg * (per + 1)
        status = torch.zeros((nseg, 4), dtype=torch.int32, device="cuda")
        entries = torch.zeros((ecap, 4), dtype=torch.int32, device="cuda")
        n_entries = torch.zeros(1, dtype=torch.int64, device="cuda")
        ctx.segment_walk(d, cap, cap, nseg, dc, status, entries, n_entries)
        ctx.check()
        n = int(n_entries.item())
        assert n == nseg * per, (n, nseg, per)
        idx = torch.arange(n, dtype=torch.int32, device="cuda")
        place = torch.stack([idx, idx % n_part], 1).contiguous()
        n_place = torch.tensor([n], dtype=torch.int64, device="cuda")
        del idx

        def call():
            ctx.recovery_append(d, cap, nseg, status, entries, n_entries, place, n_place, n_part,
                                out, out_stride, out_capacity, certs, stat)

        for _ in range(args.warmup):
            call()
        ctx.check()
        st = stat.cpu().numpy().view(np.uint32)
        heads = certs.cpu().numpy().view(np.uint32)[:, 0].astype(np.int64)
        assert (st[:, 0] == segments.SEG_OK).all() and int(st[:, 1].sum()) == n
        placed = int(heads.sum())
        assert placed == nseg * seg_len, (placed, nseg * seg_len)

        def timed(fn):
            ms = []
            for _ in range(args.calls):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                ms.append(a.elapsed_time(b))
            return ms

        # alternate the two, so that neither has the quieter half of the run
        src, dst = d[:placed], out[:placed]
        for _ in range(args.warmup):
            dst.copy_(src)
        torch.cuda.synchronize()
        app_ms, cpy_ms = [], []
        for _ in range(args.rounds):
            app_ms += timed(call)
            cpy_ms += timed(lambda: dst.copy_(src))
        ctx.check()
        app, cpy = float(np.median(app_ms)), float(np.median(cpy_ms))
        traffic = 2 * placed + 16 * n + 8 * n
        r = {"value_len": value_len, "nseg": nseg, "segment_bytes": cap, "n_part": n_part,
             "records": n, "placements": n, "placed_bytes": placed,
             "algorithmic_traffic_bytes": traffic,
             "append_ms_median": app, "append_ms_min": float(min(app_ms)),
             "append_ms_max": float(max(app_ms)),
             "memcpy_ms_median": cpy, "memcpy_ms_min": float(min(cpy_ms)),
             "memcpy_ms_max": float(max(cpy_ms)),
             "append_over_memcpy": app / cpy,
             "append_GBps_of_traffic": traffic / app / 1e6,
             "memcpy_GBps_read_plus_write": 2 * placed / cpy / 1e6,
             "calls_timed": len(app_ms), "warmup": args.warmup,
             "device": torch.cuda.get_device_name(0), "build": ramcrc.lib().ramcrc_build_info().decode()}
        results.append(r)
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, f"append_{nseg}x8MiB_v{value_len}.json"), "w") as f:
            json.dump(r, f, indent=1)
            f.write("\n")
        del status, entries, place
    ctx.close()
    print(json.dumps({"recovery_append": [
        {k: r[k] for k in ("value_len", "append_ms_median", "memcpy_ms_median", "append_over_memcpy")}
        for r in results]}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nseg", type=int, default=512)
    ap.add_argument("--values", type=lambda s: [int(v) for v in s.split(",")], default=[64, 1024, 4096])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=5, help="timed calls per round")
    ap.add_argument("--rounds", type=int, default=3, help="rounds alternating append and memcpy")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "recovery_append"))
    ap.add_argument("--time-limit", type=int, default=300, help="seconds for the GPU step")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        measure(args)
        return 0
    cmd = [sys.executable, os.path.abspath(__file__), "--child"] + sys.argv[1:]
    try:
        return subprocess.run(cmd, timeout=args.time_limit).returncode
    except subprocess.TimeoutExpired:
        print("recovery_append_bench: the GPU step exceeded its time limit", file=sys.stderr)
        return 124


if __name__ == "__main__":
    sys.exit(main())
