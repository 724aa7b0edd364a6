"""Split a rocprofv3 kernel trace (the rocpd database of `rocprofv3 --kernel-trace -d DIR ...`) by the tests of the
profiled pytest run (intervals from tools/pytest_intervals.py): which K6 kernels each test launched, and per-kernel
totals of the whole run.

    python tools/kernel_map.py DIR test_intervals.json OUT.txt
"""
import glob
import json
import re
import sqlite3
import sys
from collections import Counter, defaultdict

K6 = re.compile(r"zinv|zchol|zgemm|plus")


def short(name):
    return re.sub(r"^void ", "", name).split("(")[0].replace("spywil::", "")


def main(prof, intervals, out):
    db = sqlite3.connect(sorted(glob.glob(f"{prof}/**/*.db", recursive=True))[0])
    ks = [(s, short(k)) for k, s in db.execute("select name, start from kernels order by start")]
    tests = json.load(open(intervals))
    # the clock of the trace: the one that puts the most dispatches inside some test
    def inside(c):
        iv = [(t["t0"][c], t["t1"][c]) for t in tests]
        return sum(any(a <= s <= b for a, b in iv) for s, _ in ks[:2000])
    clock = max(range(3), key=inside)
    lines = [f"K6 kernels launched per test ({len(ks)} dispatches; launches in brackets)", ""]
    for t in tests:
        a, b = t["t0"][clock], t["t1"][clock]
        c = Counter(k for s, k in ks if a <= s <= b)
        sel = ", ".join(f"{k} [{v}]" for k, v in sorted(c.items()) if K6.search(k))
        lines.append(f"{t['id'].split('::')[-1]}: {sel}")
    lines += ["", "rocprofv3 kernel statistics of the whole run:"]
    stats = defaultdict(lambda: [0, 0])
    for name, dur in db.execute("select name, duration from kernels"):
        st = stats[short(name)[:60]]
        st[0] += 1
        st[1] += dur
    tot = sum(v[1] for v in stats.values())
    for k, (calls, dur) in sorted(stats.items(), key=lambda kv: -kv[1][1]):
        lines.append(f"{k:44s} calls {calls:6d}  total {dur / 1e6:9.3f} ms  avg {dur / calls / 1e3:9.2f} us  "
                     f"{100 * dur / tot:6.2f} %")
    open(out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(*sys.argv[1:4])
