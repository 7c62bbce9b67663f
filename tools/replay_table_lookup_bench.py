#!/usr/bin/env python3
"""Time the replay table's lookup by key (ramcrc_replay_table_lookup_device)
beside the adds that built the table and a device-to-device copy of the key
buffer.

    python tools/replay_table_lookup_bench.py [--nseg 512] [--batches 8]
                                              [--values 64,1024,4096]
                                              [--out profiles/replay_table_lookup]

The table is replay_table_bench.py's `distinct` shape: RecoverSegmentBenchmark-
shaped 8 MiB segments built on the device (fill_objects: table 0, 8-byte
counter keys), the first entry of every segment retyped to a SEGHEADER, walked
as --batches batches with the partition call's hashes and added batch by batch.
A second set of segments with later counter keys is walked and partitioned but
never added: its keys are the misses, and the partition call supplies their
hashes too.

Three query shapes, n keys each (n: the table's keys): `hits`, every key of the
table in a shuffled order; `misses`, as many keys that are not in it; `half`,
the two alternating.  In one round the calls alternate -- reset and the adds
with the given hashes, the three lookups with the given hashes, reset and the
adds with NULL hashes, the three lookups with NULL, `hits` once more with the
given hashes and without d_counts, the copy of the key buffer (torch's copy_ of
uint8 tensors, which issues hipMemcpyAsync) -- each bracketed
by device events; the medians are over --calls rounds after --warmup warm-up
rounds, and the ratios lookup / adds are taken round by round.  The yardstick
is the add of the same records with the same hashes: it makes the same probe
and three atomics per record on top.  Every run checks the counts of every
lookup and 256 sampled results of each against the live query's d_winner.  One
JSON file per value size, and one summary line each on stdout.

Each value size is measured in a child process of its own under a time limit;
this process never opens the GPU.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MiB = 1 << 20
SHAPES = ("hits", "misses", "half")


def measure(args, value_len):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import numpy as np
    import torch
    from ramcloud_amd import build, ramcrc, segments
    from replay_table_bench import Walk

    build.build()
    if not torch.cuda.is_available():
        raise SystemExit("replay_table_lookup_bench: no GPU (no fallback)")
    ctx = ramcrc.Context(0)
    cap, nseg, nb = 8 * MiB, args.nseg, args.batches
    assert nseg % nb == 0
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")

    def source(first_key):
        d = torch.empty(nseg * cap, dtype=torch.uint8, device="cuda")
        d.random_(0, 256)
        dc = z((nseg, 2), torch.int32)
        per, seg_len, _ = ctx.fill_objects(d, cap, cap, nseg, value_len, first_key=first_key, certs=dc)
        first = d.view(nseg, cap)[:, 0]
        first.copy_((first & 0xC0) | segments.LOG_ENTRY_TYPE_SEGHEADER)
        ctx.certify(d, cap, cap, nseg, torch.full((nseg,), seg_len, dtype=torch.int32, device="cuda"), dc)
        parts = [Walk(torch, ctx, segments, d, dc, cap, b * (nseg // nb), nseg // nb, per) for b in range(nb)]
        for p in parts:
            p.walk(ctx)
        return d, per, parts

    def keys_of(parts):
        """(key bytes uint8 [n, 8], hashes int64 [n], batch int32 [n], record int32 [n]) of the objects."""
        out = [[], [], [], []]
        for b, p in enumerate(parts):
            n = int(p.n_entries.item())
            e = p.entries[:n].long()
            rec = torch.nonzero((e[:, 3] & 0x3F) == segments.LOG_ENTRY_TYPE_OBJ).reshape(-1)
            e = e[rec]
            at = e[:, 0] * cap + e[:, 1] + 1 + ((e[:, 3] >> 6) & 3) + 1 + 27
            out[0].append(p.d[at[:, None] + torch.arange(8, device="cuda")])
            out[1].append(p.key_hash[rec])
            out[2].append(torch.full_like(rec, b, dtype=torch.int32))
            out[3].append(rec.int())
        return [torch.cat(x) for x in out]

    d, per, parts = source(0)
    d2, _, others = source(nseg * per)
    hit_key, hit_hash, hit_batch, hit_rec = keys_of(parts)
    miss_key, miss_hash, _, _ = keys_of(others)
    del d2, others
    n = hit_key.shape[0]
    assert n == nseg * (per - 1) == miss_key.shape[0], (n, nseg, per)
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    perm = torch.randperm(n, device="cuda", generator=g)
    hit_key, hit_hash, hit_batch, hit_rec = hit_key[perm], hit_hash[perm], hit_batch[perm], hit_rec[perm]
    miss_key, miss_hash = miss_key[perm], miss_hash[perm]
    even = torch.arange(n, device="cuda") % 2 == 0
    keybuf = {"hits": hit_key, "misses": miss_key, "half": torch.where(even[:, None], hit_key, miss_key)}
    hashes = {"hits": hit_hash, "misses": miss_hash, "half": torch.where(even, hit_hash, miss_hash)}
    keybuf = {k: v.contiguous().reshape(-1) for k, v in keybuf.items()}
    hashes = {k: v.contiguous() for k, v in hashes.items()}
    queries = z((n, 3), torch.int64)   # table 0, key_off, key_len 8 (reserved 0)
    queries[:, 1] = 8 * torch.arange(n, device="cuda")
    queries[:, 2] = 8
    results = z((n, 8), torch.int32)
    counts = z(5, torch.int64)
    copy_dst = torch.empty_like(keybuf["hits"])
    winners = [z((p.ecap, 2), torch.int32) for p in parts]
    ctx.reserve(32, max(p.ecap for p in parts))
    table = ramcrc.ReplayTable(ctx, nseg * per, nb)
    ev = lambda: torch.cuda.Event(enable_timing=True)

    def timed(fn):
        a, b = ev(), ev()
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def adds(given):
        table.reset()

        def go():
            for p in parts:
                table.add(p.d, cap, p.nseg, p.status, p.entries, p.n_entries, p.work,
                          key_hash=p.key_hash if given else None)
        return timed(go)

    def lookup(shape, given, want_counts=True):
        return timed(lambda: table.lookup(keybuf[shape], queries, results,
                                          counts=counts if want_counts else None,
                                          key_hash=hashes[shape] if given else None))

    want_counts = {"hits": (n, 0, 0, 0, 0), "misses": (0, 0, n, 0, 0),
                   "half": ((n + 1) // 2, 0, n // 2, 0, 0)}
    sample = torch.randint(0, n, (256,), device="cuda", generator=g)

    def check(shape, want_ref):
        """The counts, and 256 sampled results against the live query's d_winner."""
        assert tuple(counts.tolist()) == want_counts[shape], (shape, counts.tolist())
        r = results[sample].cpu().numpy().view(np.uint32)
        miss = np.ones(256, bool) if shape == "misses" else \
            (sample_np % 2 == 1) if shape == "half" else np.zeros(256, bool)
        assert (r[miss, 4] == segments.LOOKUP_ABSENT).all() and (r[miss, :2] == segments.RESOLVE_NONE).all()
        assert (r[~miss, 4] == segments.LOOKUP_OBJECT).all() and (r[~miss, 7] == value_len).all()
        assert np.array_equal(r[~miss, :2], want_ref[~miss]), shape

    for _ in range(args.warmup):
        for given in (True, False):
            adds(given)
            for shape in SHAPES:
                lookup(shape, given)
        copy_dst.copy_(keybuf["hits"])
    ctx.check()
    for b, p in enumerate(parts):
        table.live(b, p.live, p.n_live, p.counts, winner=winners[b])
    base = torch.tensor(np.cumsum([0] + [p.ecap for p in parts[:-1]]), device="cuda")
    want_ref = torch.cat(winners)[base[hit_batch[sample].long()] + hit_rec[sample].long()]
    want_ref = want_ref.cpu().numpy().view(np.uint32)
    sample_np = sample.cpu().numpy()
    names = ["adds_given"] + [s + "_given" for s in SHAPES] + ["adds_null"] + [s + "_null" for s in SHAPES]
    names += ["hits_given_no_counts", "memcpy"]   # d_counts = NULL: what the counters cost
    ms = {k: [] for k in names}
    for _ in range(args.calls):   # alternate, so that none has the quieter part of the run
        for given in (True, False):
            tag = "given" if given else "null"
            ms["adds_" + tag].append(adds(given))
            for shape in SHAPES:
                ms[f"{shape}_{tag}"].append(lookup(shape, given))
                check(shape, want_ref)
        ms["hits_given_no_counts"].append(lookup("hits", True, want_counts=False))
        ms["memcpy"].append(timed(lambda: copy_dst.copy_(keybuf["hits"])))
    ctx.check()
    mmm = lambda v: [round(float(np.median(v)), 4), round(min(v), 4), round(max(v), 4)]
    ratio = lambda a, b: mmm([x / y for x, y in zip(ms[a], ms[b])])
    r = {"value_len": value_len, "nseg": nseg, "batches": nb, "segment_bytes": cap,
         "keys": n, "queries": n, "key_bytes": 8, "key_buffer_bytes": 8 * n,
         "table_slots": int(2 ** int(np.ceil(np.log2(max(64, 2 * nseg * per))))),
         "calls_timed": args.calls, "warmup": args.warmup,
         "device": torch.cuda.get_device_name(0), "build": ramcrc.lib().ramcrc_build_info().decode(),
         "ms_median_min_max": {k: mmm(v) for k, v in ms.items()},
         "mkeys_per_s_median": {k: round(n / float(np.median(v)) / 1e3, 1) for k, v in ms.items()
                                if k != "memcpy"},
         # per round: a lookup of n keys over the add of the same n records with the same hashes
         "ratio_lookup_over_adds_median_min_max": {
             f"{s}_{t}": ratio(f"{s}_{t}", "adds_" + t) for t in ("given", "null") for s in SHAPES}}
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, f"lookup_{nseg}x8MiB_b{nb}_v{value_len}.json"), "w") as f:
        f.write("{\n" + ",\n".join(f" {json.dumps(k)}: {json.dumps(v)}" for k, v in r.items())
                + "\n}\n")   # one key per line
    print(json.dumps({"replay_table_lookup": dict(value_len=value_len, keys=n,
                                                  ratio=r["ratio_lookup_over_adds_median_min_max"],
                                                  **{k + "_ms": r["ms_median_min_max"][k] for k in ms})}),
          flush=True)
    table.close()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nseg", type=int, default=512)
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--values", type=lambda s: [int(v) for v in s.split(",")], default=[64, 1024, 4096])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=15, help="timed rounds")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "replay_table_lookup"))
    ap.add_argument("--time-limit", type=int, default=180, help="seconds per value size")
    ap.add_argument("--child", type=int, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child is not None:
        measure(args, args.child)
        return 0
    for value_len in args.values:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", str(value_len)] + sys.argv[1:]
        try:
            rc = subprocess.run(cmd, timeout=args.time_limit).returncode
        except subprocess.TimeoutExpired:
            print("replay_table_lookup_bench: a GPU step exceeded its time limit", file=sys.stderr)
            return 124
        if rc:
            return rc   # nothing more is started on the GPU after a failure
    return 0


if __name__ == "__main__":
    sys.exit(main())
