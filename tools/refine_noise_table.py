"""The refine-noise lines of tests/test_gpu_refine_family.py reduced to profiles/refine_noise.txt's table: per test part, schedule and
region the largest ratio of the maximum and of the mean error to the fp32 oracle's, with the case it occurred on.

    python -m pytest tests/test_gpu_refine_family.py -m gpu -s > refine_family.log
    python tools/refine_noise_table.py refine_family.log          (the table; the header of the committed file is written by hand)"""
import collections
import re
import sys

pat = re.compile(r"^[.FEsx]*refine-noise (\w+) (\S+) (?:iters\s+\d+ |k\s+\d+ )?\[(.*?)\] (\S+)\s+max hip/fp64 (\S+) fp32/fp64 (\S+) ratio\s+(\S+) \(bound (\S+)\)\s+"
                 r"mean hip/fp64 (\S+) fp32/fp64 (\S+) ratio\s+(\S+) \(bound (\S+)\)")
rows = collections.OrderedDict()
n = 0
for l in open(sys.argv[1]):
    m = pat.match(l)
    if not m:
        assert "refine-noise" not in l, l
        continue
    n += 1
    part, case, sched, region, emax, nmax, rmax, bmax, emean, nmean, rmean, bmean = m.groups()
    key = (part, sched, region)
    r = rows.setdefault(key, dict(n=0, rmax=-1.0, rmean=-1.0, bmax=bmax, bmean=bmean))
    r["n"] += 1
    if float(rmax) > r["rmax"]:
        r.update(rmax=float(rmax), cmax=case, emax=emax, nmax=nmax)
    if float(rmean) > r["rmean"]:
        r.update(rmean=float(rmean), cmean=case, emean=emean, nmean=nmean)
print(f"# {n} comparisons; one row per (test part, schedule, region): the largest ratio of the maximum and of the mean error to the fp32 oracle's,")
print("# the case it occurred on, and the two errors there (engine / fp64, fp32 oracle / fp64)")
print(f"# {'part':9s} {'schedule':22s} {'region':8s} {'n':>4s}  {'max':>6s} {'bound':>5s}  {'case':22s} {'hip':>9s} {'fp32':>9s}   {'mean':>6s} {'bound':>5s}  {'case':22s} {'hip':>9s} {'fp32':>9s}")
for (part, sched, region), r in rows.items():
    print(f"{part:11s} {sched:22s} {region:8s} {r['n']:4d}  {r['rmax']:6.2f} {r['bmax']:>5s}  {r['cmax']:22s} {r['emax']:>9s} {r['nmax']:>9s}   "
          f"{r['rmean']:6.2f} {r['bmean']:>5s}  {r['cmean']:22s} {r['emean']:>9s} {r['nmean']:>9s}")
