#!/usr/bin/env python3
"""Development probe for the ring kernel: force-kernel time per rank of a G-rank partition of N bodies on ONE GPU
(ranks serialised) for a list of kernel variants, plus the in-kernel phase stamps of the probe builds (variant 58: 2 rings x
8 waves per workgroup, 59: 4 x 4).  For every launch of a probe build the ring records are also laid out per CU, and the
time a CU's wave slots stand idle is split three ways (occupancy(), profiles/ring_queue_probe.txt).
    python3 ring_probe.py N G variants [steps] [stock]"""
import os
import sys

os.environ["NBODY_GROUP_SERIALIZE"] = "1"
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, ROOT)
import torch  # noqa: F401,E402
import numpy as np  # noqa: E402
import ppa_nbody_collisions_amd as nb  # noqa: E402

PROBE_RINGS = {58: 2, 59: 4, 63: 4}                        # rings per workgroup of the probe builds


def occupancy(ev, rings_per_wg, label):
    """One launch's ring records {first turn, end, HW_ID, XCC << 20 | ring}: where the wave slots of a CU stand idle.
    A workgroup fills its CU (16 waves of 123 VGPRs), so the workgroups of a CU run one after the other ("rounds").  Per CU,
    as shares of the launch time T = last end - first start, averaged over the CUs:
      ramp   first turn of the CU's first workgroup - first turn of the launch
      gaps   sum over successive workgroups of (first turn of the next - last ring end of the one before)
      rings  sum over workgroups of (last ring end - mean ring end): slots of rings that ended before their workgroup
      tail   end of the launch - last ring end of the CU's last workgroup
    gaps + rings + tail is what levelling across and inside CUs could recover at most (ramp is the dispatcher's)."""
    t0 = ev["step"].astype(np.int64) & 0xffffffff
    t1 = ev["i"].astype(np.int64) & 0xffffffff
    hw = ev["j"].astype(np.int64) & 0xffffffff
    kind = ev["kind"].astype(np.int64)
    place = ((kind >> 20) & 0xf) * 256 + ((hw >> 8) & 0xff)             # XCC, then SE / SH / CU of HW_ID
    wg = (kind & 0xfffff) // rings_per_wg
    begin, T = t0.min(), float(t1.max() - t0.min())
    wgs = {}
    for g in np.unique(wg):
        m = wg == g
        assert len(np.unique(place[m])) == 1, "a workgroup's rings on more than one CU"
        wgs[g] = (place[m][0], t0[m].min(), t1[m].max(), t1[m].mean(), t0[m].max() - t0[m].min())
    cus = {}
    for g, rec in wgs.items():
        cus.setdefault(rec[0], []).append(rec)
    ramp, gaps, rings, tail, rounds, gap_list = [], [], [], [], {}, []
    for recs in cus.values():
        recs.sort(key=lambda r: r[1])
        ramp.append(recs[0][1] - begin)
        g = [b[1] - a[2] for a, b in zip(recs, recs[1:])]
        gap_list += g
        gaps.append(sum(g))
        rings.append(sum(r[2] - r[3] for r in recs))
        tail.append(t1.max() - recs[-1][2])
        for k, r in enumerate(recs):
            rounds.setdefault(k, []).append(r)
    per_cu = np.bincount([len(v) for v in cus.values()])
    print("   %s: %d rings, %d workgroups on %d CUs (CUs by workgroups taken: %s); T = %d ticks (%.3f ms)" %
          (label, len(ev), len(wgs), len(cus), " ".join("%dx%d" % (c, k) for k, c in enumerate(per_cu) if c), T, T / 1e5))
    for k in sorted(rounds):
        r = rounds[k]
        ends = np.array([x[2] for x in r], dtype=np.float64)
        life = np.array([x[2] - x[1] for x in r], dtype=np.float64)
        inner = np.array([x[2] - x[3] for x in r], dtype=np.float64)
        print("     round %d: %4d workgroups; ends after launch start: min %d mean %d max %d; (slowest - mean) / T %.4f; "
              "life min %d p50 %d max %d; ring ends inside a workgroup, last - mean: mean %d max %d (%.4f of T)" %
              (k, len(r), ends.min() - begin, ends.mean() - begin, ends.max() - begin, (ends.max() - ends.mean()) / T,
               life.min(), np.percentile(life, 50), life.max(), inner.mean(), inner.max(), inner.mean() / T))
    if gap_list:
        print("     drain gaps (last ring end -> next workgroup's first turn) ticks: min %d p50 %d p90 %d max %d" %
              (min(gap_list), np.percentile(gap_list, 50), np.percentile(gap_list, 90), max(gap_list)))
    shares = [float(np.mean(x)) / T for x in (ramp, gaps, rings, tail)]
    print("     idle wave-slot time per CU / T: ramp %.4f  gaps %.4f  rings %.4f  tail %.4f;  gaps + rings + tail = %.4f "
          "(%.3f ms of this launch)" % (shares[0], shares[1], shares[2], shares[3], sum(shares[1:]), sum(shares[1:]) * T / 1e5),
          flush=True)
    return sum(shares[1:])


n, world = int(sys.argv[1]), int(sys.argv[2])
variants = [int(v) for v in sys.argv[3].split(",")]
steps = int(sys.argv[4]) if len(sys.argv) > 4 else 3
kw = {} if (len(sys.argv) > 5 and sys.argv[5] == "stock") else {"minRadius": 0.0, "maxRadius": 0.0}
cfg = nb.stock_config(particleCount=n, **kw)
bodies = nb.init_bodies(cfg)
ref = None
for variant in variants:
    grp = nb.StepperGroup(world, cfg=cfg, kernel_variant=variant)
    grp.upload(bodies)
    grp.step(1)
    s0 = [r.stats() for r in grp.ranks]
    for r in grp.ranks:
        r.set_kernel_timing(True)
    grp.step(steps)
    s1 = [r.stats() for r in grp.ranks]
    ms = [b.force_kernel_ms / max(1, b.force_kernel_launches) for b in s1]
    pairs = sum(b.pairs - a.pairs for a, b in zip(s0, s1)) / steps
    out = grp.download()
    same = ""
    if ref is None:
        ref = out.block.copy()
    else:
        same = "  bits==first: %s" % np.array_equal(ref.view(np.uint32), out.block.view(np.uint32))
    print("N=%d G=%d variant=%2d  kernel ms/rank: max %.3f min %.3f  -> %.3e pairs/s%s" %
          (n, world, variant, max(ms), min(ms), pairs / (max(ms) * 1e-3), same), flush=True)
    if max(ms) > 1.1 * min(ms):
        print("   per rank:", " ".join("%.3f" % m for m in ms), flush=True)
    if variant in PROBE_RINGS:
        p = grp.ranks[0].ring_probe()
        turns = max(1, p[5])
        ghz = p[6] / max(1, p[7]) * 0.1
        print("   probe rank0: per wave-turn cycles: evaluate %.0f  wait %.0f  chain+publish %.0f  check %.0f;"
              " polls/turn %.2f; shader clock %.2f GHz (one wave's life %.3f ms)" %
              (p[0] / turns, p[1] / turns, p[2] / turns, p[3] / turns, p[4] / turns, ghz, p[7] / 1e5), flush=True)
        ev = grp.ranks[0].events()
        if len(ev):
            t0 = ev["step"].astype(np.int64) & 0xffffffff
            t1 = ev["i"].astype(np.int64) & 0xffffffff
            base = t0.min()
            hw = ev["j"].astype(np.int64) & 0xffffffff
            xcc = (ev["kind"].astype(np.int64) >> 20) & 0xf
            cu = (hw >> 8) & 0xf
            se = (hw >> 13) & 0x7
            place = xcc * 1000 + se * 100 + cu
            print("   %d workgroup records (all launches); start ticks after first: p50 %d p90 %d max %d; "
                  "life ticks: min %d p50 %d max %d; distinct (xcc,se,cu): %d; max WGs on one CU: %d" %
                  (len(ev), np.percentile(t0 - base, 50), np.percentile(t0 - base, 90), (t0 - base).max(),
                   (t1 - t0).min(), np.percentile(t1 - t0, 50), (t1 - t0).max(), len(np.unique(place)),
                   np.bincount(np.unique(place, return_inverse=True)[1]).max()))
            last = ev[-min(len(ev), 512):]
            lt0 = (last["step"].astype(np.int64) & 0xffffffff); lt1 = (last["i"].astype(np.int64) & 0xffffffff)
            lb = lt0.min()
            print("   last launch: starts p50 %d p99 %d max %d; ends min %d p50 %d max %d (ticks after its first start)" %
                  (np.percentile(lt0 - lb, 50), np.percentile(lt0 - lb, 99), (lt0 - lb).max(), (lt1 - lb).min(),
                   np.percentile(lt1 - lb, 50), (lt1 - lb).max()))
            per_launch = len(ev) // (steps + 1)                     # one record per ring that has own bodies
            if len(ev) == per_launch * (steps + 1):                 # (the own range did not change between the launches)
                for k in range(steps + 1):
                    occupancy(ev[k * per_launch:(k + 1) * per_launch], PROBE_RINGS[variant], "rank 0 launch %d" % k)
    grp.close()
