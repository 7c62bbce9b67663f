#!/usr/bin/env python3
"""Time the build of a secondary index over the replay table
(ramcrc_replay_table_index_build_device) and the lookups in it
(ramcrc_index_lookup_device), each beside same-run references.

    python tools/replay_index_bench.py [--nseg 512] [--batches 8] [--values 64,1024]
                                       [--second 8,16,64] [--out profiles/replay_index]

The table is the README's, with one change: the replicas are built so that every
object carries a second key.  An object is {8-byte counter key, second key of
--second bytes, value}; the sizes are computed so that the 8 MiB segments still
fill.  The second key's first 8 bytes are a bijective mix of (counter >> 2), so
four objects share every 8-byte prefix: with 8-byte second keys they are equal
keys told apart by their hashes, with longer keys the comparator has to read
key bytes behind the prefix.  The first entry of every segment is retyped to a
SEGHEADER; the segments are walked as --batches batches and added batch by
batch with the partition call's hashes.

One round times, each bracketed by device events:
  build            the index build at exactly the needed capacities;
  enumerate_keys   a keys-only enumeration of the same table: the same pass
                   over the slots, its bytes copied;
  copy             a device-to-device copy of the index's bytes (entries,
                   hashes, keys: torch's copy_ of uint8 tensors);
  point_lookup     as many point queries as the index has entries, shuffled,
                   max_hashes 8;
  point_read       read_hashes of the hashes those queries returned;
  range_lookup     1,000 ranges that return n / 1000 hashes each;
  range_read       read_hashes of the hashes those ranges returned.
Medians are over --calls rounds after --warmup warm-up rounds.  Every summary
is checked: the entries against the table's keys, the order of the first
entries, the hashes returned against the entries asked for.  Where the build's
time goes (slot passes, sort passes, key copy) comes from a kernel trace of one
child of this tool in a run of its own.

One JSON file per shape, and one summary line each on stdout.  Each shape is
measured in a child process of its own under a time limit; this process never
opens the GPU.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MiB = 1 << 20
MIX = 0x9E3779B97F4A7C15   # odd: a bijection of 64-bit words


def measure(args, value_len, second_len):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import numpy as np
    import torch
    from ramcloud_amd import build, ramcrc, segments
    from replay_table_bench import Walk

    build.build()
    if not torch.cuda.is_available():
        raise SystemExit("replay_index_bench: no GPU (no fallback)")
    ctx = ramcrc.Context(0)
    cap, nseg, nb, K = 8 * MiB, args.nseg, args.batches, second_len
    assert nseg % nb == 0 and K >= 8
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")

    # the replicas: `per` equal entries a segment
    L = 24 + 1 + 4 + 8 + K + value_len          # Object::Header, KeyCount, two lengths, the keys, the value
    lb = 1 if L < 256 else 2
    E = 1 + lb + L
    per = cap // E
    d = torch.empty(nseg * cap, dtype=torch.uint8, device="cuda")
    d.random_(0, 256)
    d.view(nseg, cap)[:, per * E:] = 0
    body = torch.as_strided(d, (nseg, per, E), (cap, E, 1))
    o = 1 + lb
    body[:, :, 0] = segments.LOG_ENTRY_TYPE_OBJ | ((lb - 1) << 6)
    body[:, :, 1] = L & 255
    if lb == 2:
        body[:, :, 2] = L >> 8
    body[:, :, o:o + 24] = 0
    body[:, :, o + 8] = 1                        # version 1, table 0
    body[:, :, o + 24] = 2
    body[:, :, o + 25], body[:, :, o + 26] = 8, 0
    body[:, :, o + 27], body[:, :, o + 28] = (8 + K) & 255, (8 + K) >> 8
    shifts = 8 * torch.arange(8, device="cuda")
    for s0 in range(0, nseg, 64):                # (in slabs: the byte planes are 8 times the counters)
        s1 = min(nseg, s0 + 64)
        g = (torch.arange(s0, s1, device="cuda")[:, None] * per + torch.arange(per, device="cuda")[None, :])
        body[s0:s1, :, o + 29:o + 37] = ((g[:, :, None] >> shifts) & 255).to(torch.uint8)
        pre = (g >> 2) * torch.tensor(MIX - (1 << 64), device="cuda")   # wraps: the bijection mod 2^64
        body[s0:s1, :, o + 37:o + 45] = ((pre[:, :, None] >> shifts.flip(0)) & 255).to(torch.uint8)   # big-endian
        for k in range(8, K, 8):
            more = (g + k) * torch.tensor(MIX - (1 << 64), device="cuda")
            body[s0:s1, :, o + 37 + k:o + 45 + k] = ((more[:, :, None] >> shifts) & 255).to(torch.uint8)
        del g, pre
    first = d.view(nseg, cap)[:, 0]
    first.copy_((first & 0xC0) | segments.LOG_ENTRY_TYPE_SEGHEADER)
    dc = z((nseg, 2), torch.int32)
    ctx.certify(d, cap, cap, nseg, torch.full((nseg,), per * E, dtype=torch.int32, device="cuda"), dc)
    parts = [Walk(torch, ctx, segments, d, dc, cap, b * (nseg // nb), nseg // nb, per) for b in range(nb)]
    for p in parts:
        p.walk(ctx)
    table = ramcrc.ReplayTable(ctx, nseg * per, nb)
    for p in parts:
        table.add(p.d, cap, p.nseg, p.status, p.entries, p.n_entries, p.work, key_hash=p.key_hash)
    ctx.check()
    n = nseg * (per - 1)

    got = lambda t, dt: {k: int(v) for k, v in zip(dt.names, t.cpu().numpy().view(dt)[0])}
    b_sum, l_sum = z(7, torch.int64), z(6, torch.int64)
    table.index_build(0, 1, None, None, None, b_sum, entry_capacity=0, keys_capacity=0)
    ctx.check()
    need = got(b_sum, segments.INDEX_BUILD_SUMMARY_DTYPE)
    assert need["entries_needed"] == n and need["key_bytes_needed"] == n * K and need["objects_seen"] == n, need
    entries, hashes = torch.empty(32 * n, dtype=torch.uint8, device="cuda"), z(n, torch.int64)
    ikeys = torch.empty(n * K, dtype=torch.uint8, device="cuda")
    index_bytes = 32 * n + 8 * n + n * K
    copy_src = torch.empty(index_bytes, dtype=torch.uint8, device="cuda")
    copy_dst = torch.empty(index_bytes, dtype=torch.uint8, device="cuda")
    room = n * (4 + 24 + 1 + 4 + 8 + K)
    payload, en_summary = torch.empty(room, dtype=torch.uint8, device="cuda"), z(11, torch.int64)

    ev = lambda: torch.cuda.Event(enable_timing=True)

    def timed(fn):
        a, b = ev(), ev()
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def do_build():
        return table.index_build(0, 1, entries, hashes, ikeys, b_sum)

    index = do_build()
    ctx.check()
    s = got(b_sum, segments.INDEX_BUILD_SUMMARY_DTYPE)
    assert s["n_entries"] == n and s["key_bytes"] == n * K and not s["overflow"] and not s["spoiled"], s
    head = entries[:32 * 4096].cpu().numpy().view(segments.INDEX_ENTRY_DTYPE)
    kcpu = ikeys.cpu().numpy() if n * K < (1 << 31) else None
    order = [(int(e["prefix"]), int(e["pk_hash"])) for e in head]
    assert all(a[0] <= b[0] for a, b in zip(order, order[1:])), "the first entries' prefixes do not ascend"
    if kcpu is not None:
        full = [(kcpu[int(e["key_off"]):int(e["key_off"]) + K].tobytes(), int(e["pk_hash"])) for e in head]
        assert full == sorted(full), "the first entries are not in order"
    assert torch.equal(hashes[:4096].cpu(), torch.from_numpy(head["pk_hash"].astype(np.int64))[:4096])

    # the queries: a point query per entry, shuffled; 1,000 ranges of n / 1000 entries
    rng = np.random.default_rng(5)
    e_all = entries.cpu().numpy().view(segments.INDEX_ENTRY_DTYPE)
    pick = rng.permutation(n)
    pq = np.zeros(n, segments.INDEX_QUERY_DTYPE)
    pq["first_off"] = pq["last_off"] = e_all["key_off"][pick]
    pq["first_len"] = pq["last_len"] = K
    pq["max_hashes"] = 8
    width = n // 1000
    lo = np.arange(1000, dtype=np.int64) * width
    rq = np.zeros(1000, segments.INDEX_QUERY_DTYPE)
    rq["first_off"], rq["last_off"] = e_all["key_off"][lo], e_all["key_off"][lo + width - 1]
    rq["first_len"] = rq["last_len"] = K
    rq["first_allowed_hash"] = e_all["pk_hash"][lo]
    rq["max_hashes"] = width
    # (the queries' keys are the index's own key bytes: a second buffer of the same bytes)
    qkeys = ikeys.clone()
    d_pq = torch.from_numpy(pq.view(np.uint8).copy()).cuda().view(torch.int64)
    d_rq = torch.from_numpy(rq.view(np.uint8).copy()).cuda().view(torch.int64)
    p_out, p_res = z(8 * n, torch.int64), torch.empty(48 * n, dtype=torch.uint8, device="cuda")
    r_out, r_res = z(1000 * width, torch.int64), torch.empty(48 * 1000, dtype=torch.uint8, device="cuda")
    part = 12 + 1 + 4 + 8 + K + value_len
    reply = torch.empty(4 * n * part if 4 * n * part < (8 << 30) else 8 << 30, dtype=torch.uint8, device="cuda")
    rh_summary = z(9, torch.int64)
    del e_all

    def point_lookup():
        ctx.index_lookup(index, qkeys, d_pq, p_out, p_res, l_sum)

    def range_lookup():
        ctx.index_lookup(index, qkeys, d_rq, r_out, r_res, l_sum)

    point_lookup()
    ctx.check()
    ps = got(l_sum, segments.INDEX_LOOKUP_SUMMARY_DTYPE)
    # every key is shared by four objects at K = 8, by one otherwise
    assert ps["served"] == n and ps["bad"] == 0 and ps["n_entries"] == n and n <= ps["hashes"] <= 4 * n, ps
    range_lookup()
    ctx.check()
    rs = got(l_sum, segments.INDEX_LOOKUP_SUMMARY_DTYPE)
    assert rs["served"] == 1000 and rs["hashes"] == 1000 * width, rs
    assert torch.equal(r_out[:1000 * width], hashes[:1000 * width]), "the ranges do not tile the index"
    n_point = min(ps["hashes"], reply.numel() // part)

    def point_read():
        table.read_hashes(0, p_out, reply, rh_summary, reply.numel(), n_hashes=n_point)

    def range_read():
        table.read_hashes(0, r_out, reply, rh_summary, reply.numel(), n_hashes=1000 * width)

    def keys_only():
        table.enumerate(0, payload, en_summary, room, keys_only=True)

    def one_round():
        r = dict(build=timed(do_build), enumerate_keys=timed(keys_only),
                 copy=timed(lambda: copy_dst.copy_(copy_src)),
                 point_lookup=timed(point_lookup), point_read=timed(point_read),
                 range_lookup=timed(range_lookup), range_read=timed(range_read))
        s = got(rh_summary, segments.READ_HASHES_SUMMARY_DTYPE)
        assert s["hashes"] == 1000 * width and s["objects"] == 1000 * width, s
        s = got(en_summary, segments.ENUMERATE_SUMMARY_DTYPE)
        assert s["objects"] == n and s["full"] == 0, s
        return r

    for _ in range(args.warmup):
        one_round()
    ctx.check()
    ms = {}
    for _ in range(args.calls):
        for k, v in one_round().items():
            ms.setdefault(k, []).append(v)
    ctx.check()
    mmm = lambda v: [round(float(np.median(v)), 4), round(min(v), 4), round(max(v), 4)]
    ratio = lambda a, b: mmm([x / y for x, y in zip(ms[a], ms[b])])
    r = {"value_len": value_len, "second_key_len": K, "nseg": nseg, "batches": nb, "segment_bytes": cap,
         "entries": n, "index_bytes": index_bytes, "point_queries": n, "point_hashes": ps["hashes"],
         "point_hashes_read": n_point, "ranges": 1000, "range_hashes": 1000 * width,
         "calls_timed": args.calls, "warmup": args.warmup,
         "device": torch.cuda.get_device_name(0), "build": ramcrc.lib().ramcrc_build_info().decode(),
         "ms_median_min_max": {k: mmm(v) for k, v in ms.items()},
         "ms_rounds": {k: [round(x, 4) for x in v] for k, v in ms.items()},
         "build_entries_per_us": round(n / 1e3 / float(np.median(ms["build"])), 2),
         "ratio_build_over_enumerate_keys_median_min_max": ratio("build", "enumerate_keys"),
         "ratio_build_over_copy_median_min_max": ratio("build", "copy"),
         "ratio_point_lookup_over_point_read_median_min_max": ratio("point_lookup", "point_read"),
         "ratio_range_lookup_over_range_read_median_min_max": ratio("range_lookup", "range_read")}
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, f"index_{nseg}x8MiB_b{nb}_v{value_len}_k{K}.json"), "w") as f:
        f.write("{\n" + ",\n".join(f" {json.dumps(k)}: {json.dumps(v)}" for k, v in r.items())
                + "\n}\n")   # one key per line
    print(json.dumps({"replay_index": dict(
        value_len=value_len, second_key_len=K, entries=n, index_bytes=index_bytes,
        build_over_enumerate_keys=r["ratio_build_over_enumerate_keys_median_min_max"],
        build_over_copy=r["ratio_build_over_copy_median_min_max"],
        point_lookup_over_read=r["ratio_point_lookup_over_point_read_median_min_max"],
        range_lookup_over_read=r["ratio_range_lookup_over_range_read_median_min_max"],
        **{k + "_ms": v for k, v in r["ms_median_min_max"].items()})}), flush=True)
    table.close()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nseg", type=int, default=512)
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--values", type=lambda s: [int(v) for v in s.split(",")], default=[64, 1024])
    ap.add_argument("--second", type=lambda s: [int(v) for v in s.split(",")], default=[8, 16, 64])
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--calls", type=int, default=5, help="timed rounds")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "replay_index"))
    ap.add_argument("--time-limit", type=int, default=300, help="seconds per shape")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child is not None:
        v, k = (int(x) for x in args.child.split(","))
        measure(args, v, k)
        return 0
    for value_len in args.values:
        for second_len in args.second:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", f"{value_len},{second_len}"] + sys.argv[1:]
            try:
                rc = subprocess.run(cmd, timeout=args.time_limit).returncode
            except subprocess.TimeoutExpired:
                print("replay_index_bench: a GPU step exceeded its time limit", file=sys.stderr)
                return 124
            if rc:
                return rc   # nothing more is started on the GPU after a failure
    return 0


if __name__ == "__main__":
    sys.exit(main())
