#!/usr/bin/env python3
"""Time a multi-increment against the replay table
(ramcrc_replay_table_increment_device) beside the calls it is made of: the
lookup of the same keys, the remove of the same keys, a device-to-device copy
of exactly the output's bytes, and the write of pre-built keysAndValue images
of the same requests' new values.

    python tools/replay_table_increment_bench.py [--nseg 512] [--batches 8]
                                                 [--requests 33554432]
                                                 [--out profiles/replay_table_increment]

The table is the other replay-table benches': RecoverSegmentBenchmark-shaped
8 MiB segments built on the device (fill_objects: table 0, 8-byte counter
keys), the first entry of every segment retyped to a SEGHEADER, walked as
--batches batches and added batch by batch, every object's version set to 1
before the add.  An increment needs 8-byte values, so the table is built with
8-byte values (45-byte entries: more than twice the keys of the 64-byte
table).  The requests are --requests of its keys in a shuffled order: as many
as keep the output below 4 GiB with every key present.

Every request adds the integer 1.  Three shapes: `all_present` (table 0: a
45-byte object entry and a 42-byte tombstone entry each), `none_present` (the
same keys under table 1: a 45-byte object entry each, created from zero) and
`half` (alternating).  In one round every shape is timed five ways, each
bracketed by device events: the increment (hashes computed in the call, no
rules, d_refs, d_old and d_batch_segment_id NULL); the lookup of the same keys
(hashes computed, with counts); the remove of the same keys; a copy of the
increment's out_bytes (torch's copy_ of uint8 tensors, which issues
hipMemcpyAsync); and the write of the images of the new values.  The ratios
increment / (lookup + copy), / remove, / write and / (remove + write) are taken
round by round, and the medians are over --calls rounds after --warmup warm-up
rounds.  Every timed increment's summary is checked; once per shape the write's
output must equal the increment's byte for byte, and 256 sampled requests are
checked: the entry header, the object's fields, its new value and its checksum
against the host CRC.  The certificate is not walked here; the tests do that.
One JSON file, and one summary line on stdout.

The measurement runs in a child process of its own under a time limit; this
process never opens the GPU.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MiB = 1 << 20
SHAPES = ("all_present", "none_present", "half")
TS = 0x1AC4E3E7
VALUE_LEN = 8
OBJ_ENTRY, TOMB_ENTRY, IMAGE = 2 + 24 + 11 + 8, 2 + 32 + 8, 11 + 8


def slots_for(n):
    slots = 64
    while slots < 2 * n:
        slots *= 2
    return slots


def measure(args):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import numpy as np
    import torch
    from ramcloud_amd import build, ramcrc, segments
    from replay_table_bench import Walk

    build.build()
    if not torch.cuda.is_available():
        raise SystemExit("replay_table_increment_bench: no GPU (no fallback)")
    ctx = ramcrc.Context(0)
    cap, nseg, nb = 8 * MiB, args.nseg, args.batches
    assert nseg % nb == 0
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
    ar = lambda k: torch.arange(k, device="cuda")

    d = torch.empty(nseg * cap, dtype=torch.uint8, device="cuda")
    d.random_(0, 256)
    dc = z((nseg, 2), torch.int32)
    per, seg_len, _ = ctx.fill_objects(d, cap, cap, nseg, VALUE_LEN, first_key=0, certs=dc)
    first = d.view(nseg, cap)[:, 0]
    first.copy_((first & 0xC0) | segments.LOG_ENTRY_TYPE_SEGHEADER)
    ctx.certify(d, cap, cap, nseg, torch.full((nseg,), seg_len, dtype=torch.int32, device="cuda"), dc)
    parts = [Walk(torch, ctx, segments, d, dc, cap, b * (nseg // nb), nseg // nb, per) for b in range(nb)]
    keys, olds = [], []
    for p in parts:
        p.walk(ctx)
        e = p.entries[:int(p.n_entries.item())].long()
        e = e[(e[:, 3] & 0x3F) == segments.LOG_ENTRY_TYPE_OBJ]
        pay = e[:, 0] * cap + e[:, 1] + 1 + ((e[:, 3] >> 6) & 3) + 1
        p.d[pay + 8] = 1   # version 1
        keys.append(p.d[(pay + 27)[:, None] + ar(8)])
        olds.append(p.d[(pay + 35)[:, None] + ar(8)])
    keys, olds = torch.cat(keys), torch.cat(olds)
    n_keys = keys.shape[0]
    assert n_keys == nseg * (per - 1), (n_keys, nseg, per)
    n = min(args.requests, n_keys)
    assert n * (OBJ_ENTRY + TOMB_ENTRY) < 1 << 32, "the output of all_present must stay below 4 GiB"
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    pick = torch.randperm(n_keys, device="cuda", generator=g)[:n]
    keys, olds = keys[pick].contiguous(), olds[pick].contiguous()
    del pick
    table_of = {"all_present": z(n, torch.int64), "none_present": torch.ones(n, dtype=torch.int64, device="cuda"),
                "half": ar(n) % 2}
    tiles = (n + 255) // 256
    ctx.reserve(64 + 12 * tiles, max(8 * n + 2 * slots_for(n), max(p.ecap for p in parts)))
    table = ramcrc.ReplayTable(ctx, nseg * per, nb)
    for p in parts:
        table.add(p.d, cap, p.nseg, p.status, p.entries, p.n_entries, p.work, key_hash=None)
    ctx.check()

    kb = keys.reshape(-1)
    reqs, wreqs, images = {}, {}, {}
    for name in SHAPES:
        r = z((n, 3), torch.int64)
        r[:, 0], r[:, 1], r[:, 2] = table_of[name], 8 * ar(n), 8
        reqs[name] = r
        w = z((n, 3), torch.int64)
        w[:, 0], w[:, 1], w[:, 2] = table_of[name], IMAGE * ar(n), IMAGE
        wreqs[name] = w
        new = torch.where(table_of[name] == 0, olds.view(torch.int64).reshape(-1), 0) + 1
        img = z((n, IMAGE), torch.uint8)
        img[:, 0], img[:, 1] = 1, 8
        img[:, 3:11], img[:, 11:] = keys, new.view(torch.uint8).reshape(n, 8)
        images[name] = img.reshape(-1)
    present = {name: int((table_of[name] == 0).sum()) for name in SHAPES}
    out_bytes = {name: n * OBJ_ENTRY + present[name] * TOMB_ENTRY for name in SHAPES}
    rm_bytes = {name: present[name] * TOMB_ENTRY for name in SHAPES}
    room = max(out_bytes.values())
    out = torch.empty(room, dtype=torch.uint8, device="cuda")
    other = torch.empty(room, dtype=torch.uint8, device="cuda")   # the write's and the remove's output, the copy's
    cert, wcert = z(2, torch.int32), z(2, torch.int32)
    summary, wsum, rsum = z(18, torch.int64), z(16, torch.int64), z(12, torch.int64)
    iparts, wparts = z(5 * n, torch.int32), z(3 * n, torch.int32)
    refs = z((n, 2), torch.int32)
    args_d = z((n, 2), torch.int64)
    args_d[:, 0] = 1
    results, counts = z((n, 8), torch.int32), z(5, torch.int64)
    ev = lambda: torch.cuda.Event(enable_timing=True)
    nv = 1 << 40
    names = segments.INCREMENT_SUMMARY_DTYPE.names

    def timed(fn):
        a, b = ev(), ev()
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def want_summary(name):
        p = present[name]
        return dict(dict.fromkeys(names, 0), ok=n, created=n - p, tombstones=p, allocated=n - p,
                    next_version=nv + n - p, out_bytes=out_bytes[name], object_bytes=n * (24 + IMAGE),
                    tombstone_bytes=p * 40, value_bytes=8 * n, key_bytes=11 * n)

    def got_summary():
        s = summary.cpu().numpy().view(segments.INCREMENT_SUMMARY_DTYPE)[0]
        return {k: int(s[k]) for k in names}

    def increment(name, with_refs=False):
        table.increment(kb, reqs[name], args_d, out, cert, iparts, summary, nv, TS,
                        refs=refs if with_refs else None, out_capacity=out_bytes[name])

    def write(name):
        table.write(images[name], wreqs[name], other, wcert, wparts, wsum, nv, TS, out_capacity=out_bytes[name])

    def remove(name):
        table.remove(kb, reqs[name], other, wcert, wparts, rsum, nv, TS, out_capacity=rm_bytes[name])

    g.manual_seed(2)
    sample = torch.randint(0, n, (256,), device="cuda", generator=g)

    def check(name):
        """The write's bytes, and 256 sampled requests against the host CRC."""
        increment(name, True)
        assert got_summary() == want_summary(name), got_summary()
        write(name)
        ob = out_bytes[name]
        assert torch.equal(out[:ob], other[:ob]) and torch.equal(cert, wcert), "the write's output differs"
        r = refs.cpu().numpy().view(np.uint32)
        pp = iparts.cpu().numpy().view(np.uint8).reshape(n, 20)
        for q in sample.tolist():
            tid = int(table_of[name][q].item())
            status, version, value = (int.from_bytes(pp[q, a:b].tobytes(), "little") for a, b in ((0, 4), (4, 12), (12, 20)))
            old = int.from_bytes(olds[q].cpu().numpy().tobytes(), "little") if tid == 0 else 0
            assert status == 0 and value == (old + 1) & ((1 << 64) - 1), q
            assert (version == 2) if tid == 0 else (nv <= version < nv + n), q
            at = int(r[q, 0])
            t = out[at:at + OBJ_ENTRY].cpu().numpy().tobytes()
            assert t[0] == segments.LOG_ENTRY_TYPE_OBJ and t[1] == 24 + IMAGE, q
            tp = t[2:]
            assert tp[4:8] == TS.to_bytes(4, "little") and tp[8:16] == version.to_bytes(8, "little"), q
            assert tp[16:24] == tid.to_bytes(8, "little") and tp[24:27] == b"\x01\x08\x00", q
            assert tp[27:35] == keys[q].cpu().numpy().tobytes() and tp[35:] == value.to_bytes(8, "little"), q
            assert int.from_bytes(tp[:4], "little") == ramcrc.crc32c(tp[4:]), q
            assert (int(r[q, 1]) == at + OBJ_ENTRY) if tid == 0 else (int(r[q, 1]) == 0xFFFFFFFF), q

    def one_round(name):
        t_inc = timed(lambda: increment(name))
        assert got_summary() == want_summary(name), got_summary()
        t_look = timed(lambda: table.lookup(kb, reqs[name], results, counts=counts))
        t_remove = timed(lambda: remove(name))
        ob = out_bytes[name]
        t_copy = timed(lambda: other[:ob].copy_(out[:ob]))
        t_write = timed(lambda: write(name))
        return t_inc, t_look, t_remove, t_copy, t_write

    for name in SHAPES:
        check(name)
    ctx.check()
    for _ in range(args.warmup):
        for name in SHAPES:
            one_round(name)
    ctx.check()
    whats = ("increment", "lookup", "remove", "copy", "write")
    ms = {f"{name}_{what}": [] for name in SHAPES for what in whats}
    for _ in range(args.calls):   # alternate, so that none has the quieter part of the run
        for name in SHAPES:
            for what, t in zip(whats, one_round(name)):
                ms[f"{name}_{what}"].append(t)
    ctx.check()
    mmm = lambda v: [round(float(np.median(v)), 4), round(min(v), 4), round(max(v), 4)]
    col = lambda name: {w: ms[f"{name}_{w}"] for w in whats}
    over = {"lookup_plus_copy": lambda c, k: c["lookup"][k] + c["copy"][k], "remove": lambda c, k: c["remove"][k],
            "write": lambda c, k: c["write"][k], "remove_plus_write": lambda c, k: c["remove"][k] + c["write"][k]}
    ratio = {name: {o: mmm([col(name)["increment"][k] / f(col(name), k) for k in range(args.calls)])
                    for o, f in over.items()} for name in SHAPES}
    tag = f"{nseg}x8MiB_b{nb}_v{VALUE_LEN}"
    r = dict(value_len=VALUE_LEN, nseg=nseg, batches=nb, segment_bytes=cap, keys=n_keys, key_len=8, requests=n,
             out_bytes=out_bytes, calls_timed=args.calls, warmup=args.warmup,
             device=torch.cuda.get_device_name(0), build=ramcrc.lib().ramcrc_build_info().decode(),
             ms_median_min_max={k: mmm(v) for k, v in ms.items()},
             requests_per_us_median={name: round(n / float(np.median(ms[name + "_increment"])) / 1e3, 2)
                                     for name in SHAPES},
             # per round: the increment over the other calls of the same round
             ratio_increment_over_median_min_max=ratio)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, f"increment_{tag}.json"), "w") as f:
        f.write("{\n" + ",\n".join(f" {json.dumps(k)}: {json.dumps(v)}" for k, v in r.items())
                + "\n}\n")   # one key per line
    print(json.dumps({"replay_table_increment": dict(tag=tag, requests=n, ratio=ratio,
                                                     **{k + "_ms": r["ms_median_min_max"][k] for k in ms})}),
          flush=True)
    table.close()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nseg", type=int, default=512)
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--requests", type=int, default=1 << 25, help="at most this many of the table's keys")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=15, help="timed rounds")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "replay_table_increment"))
    ap.add_argument("--time-limit", type=int, default=300, help="seconds for the measurement")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        measure(args)
        return 0
    cmd = [sys.executable, os.path.abspath(__file__), "--child"] + sys.argv[1:]
    try:
        return subprocess.run(cmd, timeout=args.time_limit).returncode
    except subprocess.TimeoutExpired:
        print("replay_table_increment_bench: the GPU step exceeded its time limit", file=sys.stderr)
        return 124


if __name__ == "__main__":
    sys.exit(main())
