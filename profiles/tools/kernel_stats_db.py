#!/usr/bin/env python3
"""Per-kernel summary of a `rocprofv3 --kernel-trace` database (run_results.db): calls, total / mean ms, and the total
per timed chain (`--chains`: the chains the profiled bench ran, warm-up and untimed first chain included).
`python profiles/tools/kernel_stats_db.py DB [--chains N]`"""
import argparse
import re
import sqlite3

ap = argparse.ArgumentParser()
ap.add_argument("db")
ap.add_argument("--chains", type=int, default=0)
a = ap.parse_args()
con = sqlite3.connect(a.db)
rows = con.execute("select name, count(*), sum(duration) from kernels group by name order by sum(duration) desc").fetchall()
print("| kernel | calls | total ms | mean us |" + (" ms per chain |" if a.chains else ""))
print("|---|---|---|---|" + ("---|" if a.chains else ""))
for name, n, tot in rows[:12]:
    short = re.sub(r"\(.*", "", name)
    short = re.sub(r"void |9DevParams.*", "", short)
    line = f"| `{short[:90]}` | {n} | {tot / 1e6:.2f} | {tot / n / 1e3:.1f} |"
    if a.chains:
        line += f" {tot / 1e6 / a.chains:.2f} |"
    print(line)
