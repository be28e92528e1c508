#!/usr/bin/env python3
"""The host-side route queries of two builds of libldt_hip.so over fixed grids, one child process per library (no GPU): ldt_gemm_route,
ldt_score_lnfold_route and ldt_qkv_attention_route.  Prints the number of points and of differences per query; the environment (LDT_GEMM_MID=0
and the like) reaches both children.   usage: route_ab.py libA.so libB.so"""
import itertools, json, os, subprocess, sys

child = r'''
import itertools, json, os, sys
sys.path.insert(0, os.getcwd())
from ldt_amd import _lib
L = _lib.lib()
MS = (64, 77, 100, 128, 130, 1000, 1024, 1960, 2048, 3000, 4096, 5000, 8192, 10496, 16384)
NS = (64, 128, 132, 192, 256, 768, 840, 1024, 1720, 2304, 3072, 4096)
KS = (64, 72, 128, 256, 320, 1024, 2048)
out = {}
out["gemm_route"] = [L.ldt_gemm_route(e, M, N, K, N + pad, fold, wgs) for e, M, N, K, wgs, fold, pad in
                     itertools.product(range(5), MS, NS, KS, (0, 128), (0, 32, 256), (0, 4, 128))]
out["score_lnfold_route"] = [L.ldt_score_lnfold_route(M, D, F, wgs) for M, D, F, wgs in
                             itertools.product(list(range(128, 16385, 128)) + [66560], (256, 512, 768, 1024, 1280), (1024, 3072, 4096), (0, 128))]
out["qkv_attention_route"] = [L.ldt_qkv_attention_route(*p) for p in
                              itertools.product((1, 9, 10, 32, 64, 256), (32, 255, 256), (0, 32), (512, 1024), (8, 16, 32), (512, 1024), (0, 32, 256), (0, 128))]
json.dump(out, sys.stdout)
'''
dumps = []
for lib in sys.argv[1:3]:
    r = subprocess.run([sys.executable, "-c", child], env=dict(os.environ, LDT_HIP_LIB=os.path.abspath(lib)), capture_output=True, text=True, check=True)
    dumps.append(json.loads(r.stdout))
for q in dumps[0]:
    a, b = dumps[0][q], dumps[1][q]
    assert len(a) == len(b)
    print("%-20s %7d points, %d distinct answers, %d differ" % (q, len(a), len(set(a)), sum(x != y for x, y in zip(a, b))))
