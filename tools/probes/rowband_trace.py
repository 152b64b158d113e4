#!/usr/bin/env python3
"""Between two full-step attentions: wall time against the sum of the kernel durations, and one window kernel by kernel, from a rocprofv3
rocpd database (`rocprofv3 --kernel-trace -d DIR -o NAME -- python bench.py --steps 3 --warmup 1 --no-ktimer`):
    python tools/probes/rowband_trace.py DIR/**/NAME_results.db
A window = the dispatches between the end of one long attention launch (a full step's) and the start of the next.  Unbanded, the window's
kernels run one after the other (wall = sum + gaps); with row bands (rgn_rowband_fork) the two bands' kernels overlap: wall < sum, and the
listing shows band 1's kernels (other queue) starting while band 0's are still running."""
import sqlite3
import sys


def main():
    c = sqlite3.connect(sys.argv[1])
    tabs = [r[0] for r in c.execute("select name from sqlite_master where type='table'")]
    kd = next(t for t in tabs if t.startswith("rocpd_kernel_dispatch"))
    ks = next(t for t in tabs if t.startswith("rocpd_info_kernel_symbol"))
    dcols = [r[1] for r in c.execute(f"pragma table_info({kd})")]
    scols = [r[1] for r in c.execute(f"pragma table_info({ks})")]
    namecol = "display_name" if "display_name" in scols else "kernel_name"
    qcol = "queue_id" if "queue_id" in dcols else ("stream_id" if "stream_id" in dcols else "0")
    rows = c.execute(f"select d.start, d.end, d.{qcol}, s.{namecol} from {kd} d join {ks} s on d.kernel_id = s.id order by d.start").fetchall()
    rows = [(a, b, q, n.split("(")[0].replace("void rgn::", "").replace("rgn::", "")[:60]) for a, b, q, n in rows]
    long_attn = [i for i, r in enumerate(rows) if "attention" in r[3] and "combine" not in r[3] and r[1] - r[0] > 550e3]
    groups, shown = {}, set()
    for i, j in zip(long_attn[:-1], long_attn[1:]):
        while i + 1 < j and "attention" in rows[i + 1][3]:        # the attention's own remainder / combine launches belong to it
            i += 1
        win = rows[i + 1:j]
        if not win or len(win) > 24 or any("attention" in r[3] for r in win):
            continue
        n_ln = sum("ln_modulate" in r[3] for r in win)
        queues = len({r[2] for r in win})
        key = (n_ln, queues)
        wall = (rows[j][0] - rows[i][1]) / 1e3
        busy = sum(r[1] - r[0] for r in win) / 1e3
        groups.setdefault(key, []).append((wall, busy))
        if key not in shown and len(groups[key]) == 40:           # one window of every kind, well inside the run
            shown.add(key)
            t0 = rows[i][1]
            print(f"# window with {n_ln} ln_modulate launches on {queues} queue(s): wall {wall:.1f} us, sum of kernel durations {busy:.1f} us"
                  " (start / end in us after the attention before it)")
            for a, b, q, n in win:
                print(f"  queue {q!s:>4}  {(a - t0) / 1e3:9.1f} {(b - t0) / 1e3:9.1f}  {(b - a) / 1e3:8.1f} us  {n}")
    print("# all windows between two full-step attentions: (ln_modulate launches, queues) -> count, mean wall us, mean sum of durations us")
    for key in sorted(groups):
        v = groups[key]
        print(f"  {key}: n {len(v):5d}  wall {sum(w for w, _ in v) / len(v):8.1f}  sum {sum(b for _, b in v) / len(v):8.1f}")


if __name__ == "__main__":
    main()
