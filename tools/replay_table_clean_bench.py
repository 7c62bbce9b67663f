#!/usr/bin/env python3
"""Time cleaning batches out of the replay table
(ramcrc_replay_table_clean_device) beside two things the library could
already do: the live query of the same batches followed by
ramcrc_recovery_append_device at one partition over the same lists -- the copy
without the table update --, and a device-to-device copy of exactly the
survivor's bytes.  ramcrc_replay_table_clean_size_device is timed alone.

    python tools/replay_table_clean_bench.py [--nseg 512] [--batches 8]
                                             [--victims 4]
                                             [--values 64,1024,4096]
                                             [--out profiles/replay_table_clean]

The table is replay_table_remove_bench.py's: RecoverSegmentBenchmark-shaped
8 MiB segments built on the device (fill_objects: table 0, 8-byte counter
keys), the first entry of every segment retyped to a SEGHEADER, walked as
--batches batches and added batch by batch, every object's version set to 1
before the add.  The victims are the first --victims batches.

Three shapes.  `all`: every record of the victims is live.  `half` and
`tenth`: one more batch is added for the purpose, a copy of the victims'
segments in which every second object (nine of ten) carries version 2 and so
replaces the victim's; the others tie with the victim's at version 1 and lose
to the lower batch number, so that live and dead records interleave.

A clean changes the table, so every round builds it again (reset, the adds),
then times, each bracketed by device events: clean_size; live + append of
every victim; the clean (d_moved and d_usage given); the copy of out_bytes
(torch's copy_ of uint8 tensors, which issues hipMemcpyAsync).  Ratios are
taken round by round, medians over --calls rounds after --warmup warm-up
rounds.  Every timed clean's summary is checked against clean_size's, and
once per shape 256 sampled keys are looked up after a clean: an object of
version 1 lies in the survivor batch, one of version 2 in the added copy.  The
certificate and the record table are not walked here; the tests do that.  One
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
SHAPES = {"all": 0, "half": 2, "tenth": 10}   # of every k objects one stays live (0: all)


def measure(args, value_len):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import numpy as np
    import torch
    from ramcloud_amd import build, ramcrc, segments
    from replay_table_bench import Walk

    build.build()
    if not torch.cuda.is_available():
        raise SystemExit("replay_table_clean_bench: no GPU (no fallback)")
    ctx = ramcrc.Context(0)
    cap, nseg, nb, nv = 8 * MiB, args.nseg, args.batches, args.victims
    assert nseg % nb == 0 and 0 < nv < nb
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
    ar = lambda k: torch.arange(k, device="cuda")
    ev = lambda: torch.cuda.Event(enable_timing=True)

    def timed(fn):
        a, b = ev(), ev()
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    d = torch.empty(nseg * cap, dtype=torch.uint8, device="cuda")
    d.random_(0, 256)
    dc = z((nseg, 2), torch.int32)
    per, seg_len, _ = ctx.fill_objects(d, cap, cap, nseg, value_len, first_key=0, certs=dc)
    first = d.view(nseg, cap)[:, 0]
    first.copy_((first & 0xC0) | segments.LOG_ENTRY_TYPE_SEGHEADER)
    ctx.certify(d, cap, cap, nseg, torch.full((nseg,), seg_len, dtype=torch.int32, device="cuda"), dc)
    sb = nseg // nb
    parts = [Walk(torch, ctx, segments, d, dc, cap, b * sb, sb, per) for b in range(nb)]

    def versions(p, pick=None, value=1):
        """Set the version byte of p's objects (pick: a mask over them); returns their keys."""
        e = p.entries[:int(p.n_entries.item())].long()
        e = e[(e[:, 3] & 0x3F) == segments.LOG_ENTRY_TYPE_OBJ]
        pay = e[:, 0] * cap + e[:, 1] + 1 + ((e[:, 3] >> 6) & 3) + 1
        if pick is not None:
            pay = pay[pick(pay.shape[0])]
        p.d[pay + 8] = value
        return p.d[(pay + 27)[:, None] + ar(8)]

    keys = []
    for p in parts:
        p.walk(ctx)
        k = versions(p)
        if len(keys) < nv:
            keys.append(k)
    keys = torch.cat(keys)
    n_vic = keys.shape[0]
    assert n_vic == nv * sb * (per - 1)
    victims = list(range(nv))
    vic_bytes = -(-(nv * sb * seg_len) // 16) * 16   # (always enough: the victims' certificate lengths)
    assert vic_bytes < 1 << 32
    ecap_out = sum(parts[b].ecap for b in victims)
    ctx.reserve(max(ramcrc.ReplayTable.clean_reserve([parts[b].ecap for b in victims]), 80 + 4 * sb),
                max(p.ecap for p in parts))
    table = ramcrc.ReplayTable(ctx, nseg * per + 64, nb + 2)

    out = torch.empty(vic_bytes, dtype=torch.uint8, device="cuda")
    copy_dst = torch.empty(vic_bytes, dtype=torch.uint8, device="cuda")
    o_cert, o_status, o_n = z(2, torch.int32), z((1, 4), torch.int32), z(1, torch.int64)
    o_entries, o_work, o_moved = z((ecap_out, 4), torch.int32), z(ecap_out, torch.int64), z((ecap_out, 2), torch.int32)
    usage, summary, size_summary = z((nv, 4), torch.int64), z(14, torch.int64), z(14, torch.int64)
    app_out = torch.empty(sb * cap, dtype=torch.uint8, device="cuda")   # one victim's recovery segments at a time
    app_certs, app_stat = z((sb, 2), torch.int32), z((sb, 2), torch.int32)
    names = segments.CLEAN_SUMMARY_DTYPE.names
    as_dict = lambda t: {k: int(v) for k, v in zip(names, t.cpu().numpy().view(np.uint64))}

    results = {}
    for shape, k in SHAPES.items():
        killer = None
        if k:
            # the victims' segments again, nine of ten (every second) object at version 2
            kd = d[:nv * sb * cap].clone()
            killer = Walk(torch, ctx, segments, kd, dc[:nv * sb].clone(), cap, 0, nv * sb, per)
            killer.walk(ctx)
            versions(killer, lambda m: ar(m) % k != 0, 2)
            ctx.check()

        def rebuild():
            table.reset()
            for p in parts:
                table.add(p.d, cap, p.nseg, p.status, p.entries, p.n_entries, p.work, key_hash=None)
            if killer is not None:
                table.add(killer.d, cap, killer.nseg, killer.status, killer.entries, killer.n_entries, killer.work,
                          key_hash=None)

        def live_append():
            for b in victims:
                p = parts[b]
                table.live(b, p.live, p.n_live, p.counts)
                ctx.recovery_append(p.d, cap, p.nseg, p.status, p.entries, p.n_entries, p.live, p.n_live, 1,
                                    app_out, cap, cap, app_certs, app_stat)

        def clean():
            return table.clean(victims, out, o_cert, o_status, o_entries, o_n, o_work, summary, moved=o_moved,
                               usage=usage, out_capacity=vic_bytes)

        def one_round(check=False):
            rebuild()
            ctx.check()
            t_size = timed(lambda: table.clean_size(victims, size_summary))
            want = as_dict(size_summary)
            t_la = timed(live_append)
            t_clean = timed(clean)
            ctx.check()
            got = as_dict(summary)
            assert got == dict(want, batch=nb + (killer is not None)), (got, want)
            ob = got["out_bytes"]
            t_copy = timed(lambda: copy_dst[:ob].copy_(out[:ob]))
            if check:
                n_live = n_vic if not k else (n_vic + k - 1) // k   # (roughly: the pick runs per batch)
                assert abs(got["moved_objects"] - n_live) <= nv * sb and got["dropped_other"] == nv * sb, got
                assert got["dropped_objects"] == n_vic - got["moved_objects"] and got["moved_tombstones"] == 0
                assert int(o_cert[0].item()) & 0xFFFFFFFF == ob and int(o_n.item()) == got["needed_records"]
                g = torch.Generator(device="cuda")
                g.manual_seed(3)
                sample = torch.randint(0, n_vic, (256,), device="cuda", generator=g)
                kb = keys[sample].reshape(-1).contiguous()
                q = z((256, 3), torch.int64)
                q[:, 1], q[:, 2] = 8 * ar(256), 8
                res = z((256, 8), torch.int32)
                table.lookup(kb, q, res)
                ctx.check()
                r = res.cpu().numpy().view(segments.LOOKUP_RESULT_DTYPE).reshape(-1)
                assert (r["kind"] == segments.LOOKUP_OBJECT).all()
                moved = r["version"] == 1
                assert (r["batch"][moved] == got["batch"]).all() and (r["batch"][~moved] == nb).all()
                assert moved.any() and (not k or (~moved).any())
            return dict(clean=t_clean, live_append=t_la, copy=t_copy, clean_size=t_size), got

        _, got = one_round(check=True)
        for _ in range(args.warmup):
            one_round()
        ms = {w: [] for w in ("clean", "live_append", "copy", "clean_size")}
        for _ in range(args.calls):
            t, got = one_round()
            for w in ms:
                ms[w].append(t[w])
        mmm = lambda v: [round(float(np.median(v)), 4), round(min(v), 4), round(max(v), 4)]
        results[shape] = dict(
            summary=got, ms_median_min_max={w: mmm(v) for w, v in ms.items()},
            survivor_gb_per_s_median=round(got["out_bytes"] / float(np.median(ms["clean"])) / 1e6, 1),
            ratio_clean_over_live_append_median_min_max=mmm([c / a for c, a in zip(ms["clean"], ms["live_append"])]),
            ratio_clean_over_copy_median_min_max=mmm([c / a for c, a in zip(ms["clean"], ms["copy"])]),
            ratio_clean_size_over_clean_median_min_max=mmm([s / c for s, c in zip(ms["clean_size"], ms["clean"])]))
        del killer
    tag = f"{nseg}x8MiB_b{nb}_v{value_len}"
    r = dict(value_len=value_len, nseg=nseg, batches=nb, victims=nv, segment_bytes=cap, victim_records=n_vic + nv * sb,
             victim_bytes=vic_bytes, calls_timed=args.calls, warmup=args.warmup,
             device=torch.cuda.get_device_name(0), build=ramcrc.lib().ramcrc_build_info().decode(), shapes=results)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, f"clean_{tag}.json"), "w") as f:
        f.write("{\n" + ",\n".join(f" {json.dumps(k)}: {json.dumps(v)}" for k, v in r.items())
                + "\n}\n")   # one key per line
    print(json.dumps({"replay_table_clean": dict(
        tag=tag, **{s: dict(ms=v["ms_median_min_max"], over_live_append=v["ratio_clean_over_live_append_median_min_max"],
                            over_copy=v["ratio_clean_over_copy_median_min_max"], out_bytes=v["summary"]["out_bytes"])
                    for s, v in results.items()})}), flush=True)
    table.close()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nseg", type=int, default=512)
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--victims", type=int, default=4)
    ap.add_argument("--values", type=lambda s: [int(v) for v in s.split(",") if v], default=[64, 1024, 4096])
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--calls", type=int, default=7, help="timed rounds")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "replay_table_clean"))
    ap.add_argument("--time-limit", type=int, default=240, help="seconds per value size")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child is not None:
        measure(args, int(args.child))
        return 0
    for line in [str(v) for v in args.values]:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", line] + sys.argv[1:]
        try:
            rc = subprocess.run(cmd, timeout=args.time_limit).returncode
        except subprocess.TimeoutExpired:
            print("replay_table_clean_bench: a GPU step exceeded its time limit", file=sys.stderr)
            return 124
        if rc:
            return rc   # nothing more is started on the GPU after a failure
    return 0


if __name__ == "__main__":
    sys.exit(main())
