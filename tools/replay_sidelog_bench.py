#!/usr/bin/env python3
"""Time ramcrc_replay_sidelog_device against ramcrc_recovery_append_device on
the same list (n_part = 1) and against a device-to-device copy of the same
bytes, in one run.

    python tools/replay_sidelog_bench.py [--nseg 512] [--shapes v64,v1024,v4096,tomb,half]
                                         [--out profiles/replay_sidelog]

Shapes:
  v64, v1024, v4096  RecoverSegmentBenchmark-shaped 8 MiB segments built on the
                     device (fill_objects), no tombstones: what the references
                     and counters alone cost over the plain append;
  tomb               segments of 42-byte tombstone entries (8-byte keys);
  half               a tombstone and an object of a 64-byte value in turn:
                     what the rewrite costs.  A few segments are built on the
                     host, replicated across the batch and certified and
                     walked on the device.
Every record is kept.  After the warm-up rounds every round times one call of
each of the three, bracketed by device events, in alternation; the ratio to
the plain append is taken round by round.  The yardstick is the plain append
of the same run.  Each shape checks d_counts and a sample of the outputs (the
rewritten tombstones' checksums with the oracle's CRC32C).  One JSON file per
shape, and one summary line on stdout.

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
TS = 0x65A1B2C3
HOST_SEGMENTS = 4


def host_segments(np, kind, cap, seed):
    """HOST_SEGMENTS segments of fixed-size entries with random payloads:
    (bytes uint8 [HOST_SEGMENTS, cap], head, tombstones, objects per segment)."""
    tomb, obj = 2 + 40, 2 + 24 + 1 + 2 + 8 + 64
    unit = tomb if kind == "tomb" else tomb + obj
    n = cap // unit
    rng = np.random.default_rng(seed)
    segs = np.zeros((HOST_SEGMENTS, cap), np.uint8)
    for s in range(HOST_SEGMENTS):
        e = rng.integers(0, 256, (n, unit), dtype=np.uint8)
        e[:, 0], e[:, 1] = 3, 40                       # OBJTOMB, one length byte
        if kind == "half":
            e[:, tomb], e[:, tomb + 1] = 2, obj - 2    # OBJ
        segs[s, :n * unit] = e.reshape(-1)
    return segs, n * unit, n, n if kind == "half" else 0


def measure(args):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from oracle import oracle
    from ramcloud_amd import build, ramcrc, segments

    build.build()
    if not torch.cuda.is_available():
        raise SystemExit("replay_sidelog_bench: no GPU (no fallback)")
    ctx = ramcrc.Context(0)
    cap, nseg = 8 * MiB, args.nseg
    d = torch.empty(nseg * cap, dtype=torch.uint8, device="cuda")
    out = torch.empty(nseg * cap, dtype=torch.uint8, device="cuda")
    certs = torch.zeros((nseg, 2), dtype=torch.int32, device="cuda")
    stat = torch.zeros((nseg, 2), dtype=torch.int32, device="cuda")
    counts = torch.zeros(7, dtype=torch.int64, device="cuda")
    results = []
    for shape in args.shapes:
        dc = torch.zeros((nseg, 2), dtype=torch.int32, device="cuda")
        if shape.startswith("v"):
            d.random_(0, 256)
            per, seg_len, _ = ctx.fill_objects(d, cap, cap, nseg, int(shape[1:]), certs=dc)
            n_tomb = 0
        else:
            segs, seg_len, t_per, o_per = host_segments(np, shape, cap, 41)
            hs = torch.from_numpy(segs).cuda()
            d.view(nseg, cap).copy_(hs.repeat((nseg + HOST_SEGMENTS - 1) // HOST_SEGMENTS, 1)[:nseg])
            heads = torch.full((nseg,), seg_len, dtype=torch.int32, device="cuda")
            ctx.certify(d, cap, cap, nseg, heads, dc)
            per, n_tomb = t_per + o_per, nseg * t_per
            del hs, heads
        ecap = nseg * (per + 1)
        status = torch.zeros((nseg, 4), dtype=torch.int32, device="cuda")
        entries = torch.zeros((ecap, 4), dtype=torch.int32, device="cuda")
        n_entries = torch.zeros(1, dtype=torch.int64, device="cuda")
        ctx.segment_walk(d, cap, cap, nseg, dc, status, entries, n_entries)
        ctx.check()
        n = int(n_entries.item())
        assert n == nseg * per, (n, nseg, per)
        idx = torch.arange(n, dtype=torch.int32, device="cuda")
        live = torch.stack([idx, torch.zeros_like(idx)], 1).contiguous()
        n_live = torch.tensor([n], dtype=torch.int64, device="cuda")
        refs = torch.zeros((n, 2), dtype=torch.int32, device="cuda")
        del idx

        def sidelog():
            ctx.replay_sidelog(d, cap, nseg, status, entries, n_entries, live, n_live, TS, out, cap, cap,
                               certs, stat, counts, refs=refs)

        def append():
            ctx.recovery_append(d, cap, nseg, status, entries, n_entries, live, n_live, 1, out, cap,
                                cap, certs, stat)

        placed = nseg * seg_len
        src, dst = d[:placed], out[:placed]

        def timed(fn):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            return a.elapsed_time(b)

        sl_ms, app_ms, cpy_ms = [], [], []
        for rnd in range(args.warmup + args.rounds):
            t = (timed(sidelog), timed(append), timed(lambda: dst.copy_(src)))
            if rnd >= args.warmup:
                sl_ms.append(t[0])
                app_ms.append(t[1])
                cpy_ms.append(t[2])
        ctx.check()

        # the last side log's results: counters, then a sample of the outputs
        sidelog()
        ctx.check()
        c = counts.cpu().numpy().view(segments.SIDELOG_COUNTS_DTYPE)[0]
        tab = entries[:n].cpu().numpy().view(np.uint32)
        lens = tab[:, 2].astype(np.int64)
        is_tomb = (tab[:, 3] & 0x3F) == segments.LOG_ENTRY_TYPE_OBJTOMB
        assert int(is_tomb.sum()) == n_tomb
        want = dict(objects=n - n_tomb, tombstones=n_tomb, other=0,
                    object_bytes=int(lens[~is_tomb].sum()), tombstone_bytes=int(lens[is_tomb].sum()),
                    short_tombstones=0, left_out=0)
        got = {k: int(c[k]) for k in want}
        assert got == want, (got, want)
        heads = certs.cpu().numpy().view(np.uint32)[:, 0].astype(np.int64)
        assert int(heads.sum()) == placed, (int(heads.sum()), placed)
        rng = np.random.default_rng(43)
        sample = rng.integers(0, n, 256)
        rf = refs[torch.from_numpy(sample).cuda()].cpu().numpy().view(np.uint32)
        for i, (seg, off) in zip(sample.tolist(), rf.tolist()):
            s, so, ln, hdr = (int(v) for v in tab[i])
            lb = 1 if ln < 256 else 2 if ln < 65536 else 3
            assert seg == s
            got_e = out[seg * cap + off:seg * cap + off + 1 + lb + ln].cpu().numpy()
            sp = s * cap + so + 1 + ((hdr >> 6) & 3) + 1
            pay = bytearray(d[sp:sp + ln].cpu().numpy().tobytes())
            assert got_e[0] == (hdr & 0x3F) | ((lb - 1) << 6)
            assert int.from_bytes(got_e[1:1 + lb].tobytes(), "little") == ln
            if hdr & 0x3F == segments.LOG_ENTRY_TYPE_OBJTOMB:
                pay[8:16] = bytes(8)
                pay[24:28] = TS.to_bytes(4, "little")
                crc = oracle.crc32c(np.frombuffer(bytes(pay[:28]) + bytes(pay[32:]), np.uint8))
                pay[28:32] = int(crc).to_bytes(4, "little")
            assert got_e[1 + lb:].tobytes() == bytes(pay), ("sample", i)

        ratio = [a / b for a, b in zip(sl_ms, app_ms)]
        med = lambda v: float(np.median(v))
        # bytes the algorithm moves per record on top of the append's (which
        # reads and writes every placed byte, 16 B of record, 8 B of list, and
        # writes and reads 4 B of destination): the pass reads the destination,
        # the list and the record again and writes a reference; per tombstone
        # it reads the output bytes its checksum covers and not replaced, and
        # stores 16 bytes.
        per_record = 4 + 8 + 16 + 8
        per_tomb = (40 - 4 - 12) + 16
        r = {"shape": shape, "nseg": nseg, "segment_bytes": cap, "records": n, "tombstones": n_tomb,
             "placed_bytes": placed,
             "sidelog_ms_median": med(sl_ms), "sidelog_ms_min": float(min(sl_ms)),
             "sidelog_ms_max": float(max(sl_ms)),
             "append_ms_median": med(app_ms), "append_ms_min": float(min(app_ms)),
             "append_ms_max": float(max(app_ms)),
             "memcpy_ms_median": med(cpy_ms), "memcpy_ms_min": float(min(cpy_ms)),
             "memcpy_ms_max": float(max(cpy_ms)),
             "sidelog_over_append_median": med(ratio), "sidelog_over_append_min": float(min(ratio)),
             "sidelog_over_append_max": float(max(ratio)),
             "sidelog_over_memcpy": med(sl_ms) / med(cpy_ms),
             "append_traffic_bytes": 2 * placed + (16 + 8 + 4 + 4) * n,
             "pass_traffic_bytes": per_record * n + per_tomb * n_tomb,
             "pass_traffic_bytes_per_record": per_record, "pass_traffic_bytes_per_tombstone": per_tomb,
             "sidelog_ms": sl_ms, "append_ms": app_ms, "memcpy_ms": cpy_ms,
             "rounds": args.rounds, "warmup": args.warmup, "sampled_outputs": int(sample.size),
             "device": torch.cuda.get_device_name(0), "build": ramcrc.lib().ramcrc_build_info().decode()}
        results.append(r)
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, f"sidelog_{nseg}x8MiB_{shape}.json"), "w") as f:
            json.dump(r, f, indent=1)
            f.write("\n")
        del status, entries, live, refs, tab
    ctx.close()
    print(json.dumps({"replay_sidelog": [
        {k: r[k] for k in ("shape", "sidelog_ms_median", "append_ms_median", "memcpy_ms_median",
                           "sidelog_over_append_median")} for r in results]}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nseg", type=int, default=512)
    ap.add_argument("--shapes", type=lambda s: s.split(","), default=["v64", "v1024", "v4096", "tomb", "half"])
    ap.add_argument("--warmup", type=int, default=2, help="warm-up rounds")
    ap.add_argument("--rounds", type=int, default=15, help="timed rounds, one call of each per round")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "replay_sidelog"))
    ap.add_argument("--time-limit", type=int, default=540, help="seconds for the GPU step")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        measure(args)
        return 0
    cmd = [sys.executable, os.path.abspath(__file__), "--child"] + sys.argv[1:]
    try:
        return subprocess.run(cmd, timeout=args.time_limit).returncode
    except subprocess.TimeoutExpired:
        print("replay_sidelog_bench: the GPU step exceeded its time limit", file=sys.stderr)
        return 124


if __name__ == "__main__":
    sys.exit(main())
