"""The gap between consecutive k_sweep launches in a rocprofv3 --kernel-trace result (rocpd sqlite): gap = start(k_sweep i+1) - end(k_sweep i)
over the last `last` gaps of the run (the benchmark's timed iterations), with the k_sweep durations and the kernels inside a gap.  Every kernel whose name begins with k_sweep counts as the sweep (k_sweep_few, k_sweep_sp,
k_sweep_w, k_sweep_stream: a run launches one of them).
Usage: python tools/sweep_gap.py <results.db> [label [last = 100]]"""
import sqlite3
import sys


def pct(v, p):
    s = sorted(v)
    return s[min(len(s) - 1, max(0, int(round(p / 100.0 * (len(s) - 1)))))]


def main():
    db = sqlite3.connect(sys.argv[1])
    label = sys.argv[2] if len(sys.argv) > 2 else "run"
    last = int(sys.argv[3]) if len(sys.argv) > 3 else 100
    cols = [r[1] for r in db.execute("pragma table_info(kernels)")]
    name_col = "name" if "name" in cols else [c for c in cols if "name" in c][0]
    rows = db.execute(f"select {name_col}, start, end from kernels order by start").fetchall()
    sweeps = [(s, e) for n, s, e in rows if n.startswith("k_sweep") or "::k_sweep" in n or n.split("(")[0].endswith("k_sweep")]
    if len(sweeps) < last + 1:
        print(f"{label}: only {len(sweeps)} k_sweep launches")
        return
    tail = sweeps[-(last + 1):]
    gaps = [(tail[i + 1][0] - tail[i][1]) / 1e3 for i in range(last)]
    durs = [(e - s) / 1e3 for s, e in tail[1:]]
    per = [(tail[i + 1][0] - tail[i][0]) / 1e3 for i in range(last)]
    print(f"{label}: {len(sweeps)} k_sweep launches; gap median {pct(gaps, 50):.1f} us (p10 {pct(gaps, 10):.1f}, p90 {pct(gaps, 90):.1f}); "
          f"k_sweep median {pct(durs, 50):.1f} us (p10 {pct(durs, 10):.1f}, p90 {pct(durs, 90):.1f}); period median {pct(per, 50):.1f} us")
    inside = {}
    t0, t1 = tail[0][1], tail[-1][0]
    for n, s, e in rows:
        if t0 <= s <= t1 and not (n.startswith("k_sweep") or n.split("(")[0].endswith("k_sweep")):
            inside.setdefault(n.split("(")[0][:48], []).append((e - s) / 1e3)
    print("  kernels inside the gaps, median us (launches): " + ", ".join(f"{k} {pct(v, 50):.1f} ({len(v)})" for k, v in sorted(inside.items())))


if __name__ == "__main__":
    main()
