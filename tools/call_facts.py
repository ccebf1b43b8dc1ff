"""What the calls of a depth plan launch (the per-launch profile's names, in order, no times) and what the plan says of itself
(flatgfa_dev_plan_describe), for bench workloads and seeded random graphs -- to be diffed between two builds of the library
(FLATGFA_LIB=pollen_amd/lib_prev/libflatgfa.so) or two settings of a test hook.  The plan is made with
FLATGFA_DEPTH_PATH=bucketed FLATGFA_BIG_GROUPS=1 FLATGFA_ACC_OWN=0 (set here unless the caller set them), so that no timed
trial decides anything; then, per graph: seg_depth with unique depth, the same again (on the kept records where the plan
keeps them), seg_depth without, path_depth_all, and seg_depth with unique depth behind a status().
    python3 tools/call_facts.py [--random] [workloads...]      (default: tools/plan_facts.py's spread of shapes + its 40 random
                                                                graphs; --random: the random graphs behind the named workloads)"""
import os, sys
for k, v in (("FLATGFA_DEPTH_PATH", "bucketed"), ("FLATGFA_BIG_GROUPS", "1"), ("FLATGFA_ACC_OWN", "0")):
    os.environ.setdefault(k, v)
import numpy as np
import torch
sys.path.insert(0, ".")
import pollen_amd as pa
from pollen_amd import device as dev
from bench import WORKLOADS
sys.path.insert(0, "tools")
from fuzz_gpu import random_graph


def facts(label, graph):
    S, P = graph.n_segs, graph.n_paths
    d, u = (torch.empty(S, dtype=torch.int32, device="cuda:0") for _ in range(2))
    ln, wt = (torch.empty(P, dtype=torch.int64, device="cuda:0") for _ in range(2))
    plan = dev.DepthPlan(graph)
    calls = (("uniq", lambda: plan.seg_depth(d, u)), ("uniq again", lambda: plan.seg_depth(d, u)), ("depth", lambda: plan.seg_depth(d)),
             ("path_depth_all", lambda: plan.path_depth_all(d, ln, wt)), ("uniq after status", lambda: plan.seg_depth(d, u)))
    def status():
        try:
            plan.status()
        except pa.FlatGFAError as e:  # (a call that was not complete, a plan that had to change: a fact like the others)
            print(f"{label}: status: {e}", flush=True)
    for what, call in calls:
        if what == "uniq after status":
            status()
        dev.profile_read()
        dev.profile_enable(True)
        try:
            call()
            torch.cuda.synchronize()
        finally:
            dev.profile_enable(False)
        print(f"{label}: {what}: {' '.join(name for name, _ in dev.profile_read())}", flush=True)
    print(f"{label}: {plan.describe()}", flush=True)
    status()
    plan.close()


args = [a for a in sys.argv[1:] if not a.startswith("--")]
wls = args or ["cfgS", "cfgM", "cfgL", "cfgL-short", "cfgL-medium", "cfgL-4paths", "cfgL-fewlong", "cfgL-chrom", "chrom-1k", "hap-1k", "hap-10k",
               "hap-chr20", "rep-chr20", "cfgL-4Mseg", "tiny-paths"]
for wl in wls:
    S, P, L, model = WORKLOADS[wl]
    g = pa.synth(1, S, P, L, model, False)
    steps, pb, pe, seg_len = g.soa()
    facts(wl, dev.DeviceGraph(steps, pb, pe, S, seg_len, device="cuda:0"))
    del g
if not args or "--random" in sys.argv:
    rng = np.random.default_rng(20261003)
    for k in range(40):
        S, P, steps, pb, pe = random_graph(rng)
        facts(f"random {k} (S={S} P={P} N={len(steps)})", dev.DeviceGraph(steps, pb, pe, S, np.ones(S, dtype=np.uint32), device="cuda:0"))
