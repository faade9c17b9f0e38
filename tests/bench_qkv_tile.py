"""Developer tool: the encoder's QKV projection launch (EPI_QKV, so400m: N = 3456, K = 1152, 16 heads of 72 stored 80 wide)
at the bench batch, HIP events round every launch, 3 x 20 launches per process.  Prints one JSON line: per round the best and
the median launch in microseconds, and the median of the three round medians.  Compare two builds (SGL_LIB_PATH) or two tiles
(SGL_NT_TILE=256|288) with alternating processes in one job: the switch and the library are read once per process.
"nocheck" skips the look at the output (a main-loop-only run of the developer library, SGL_NT6_SKIP_EPI, writes none).
   python tests/bench_qkv_tile.py [B] [label] [nocheck]"""
import json, math, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import __graft_entry__ as g
pkg = g.load_package(); lib = pkg.lib.load()
B = int(sys.argv[1]) if len(sys.argv) > 1 else 128
label = sys.argv[2] if len(sys.argv) > 2 else ""
N_tok, H, hd, hdp, D = 729, 16, 72, 80, 1152
M, N, K = B * N_tok, 3 * D, D
st = torch.cuda.current_stream()
torch.manual_seed(0)
A = torch.randn(M, K, device="cuda").bfloat16(); W = (torch.randn(N, K, device="cuda") / math.sqrt(K)).bfloat16()
bias = torch.randn(N, device="cuda")
out = torch.full((3 * B * H * N_tok * hdp,), float("nan"), device="cuda", dtype=torch.bfloat16)
def f():
    rc = lib.sgl_op_gemm_nt(1, A.data_ptr(), K, W.data_ptr(), K, M, N, K, 3, out.data_ptr(), 0, None, 0, bias.data_ptr(), None, 0,
                            None, 0, None, 1, N_tok, H, hd, hdp, B, st.cuda_stream)
    assert rc == 0, rc
for _ in range(5): f()
torch.cuda.synchronize()
q = out.view(3, B, H, N_tok, hdp)
assert (len(sys.argv) > 3 and sys.argv[3] == "nocheck") or not torch.isnan(q.float()).any() and float(q[..., hd:].float().abs().max()) == 0.0
rounds = []
for r in range(3):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(20)]
    for e0, e1 in ev:
        e0.record(st); f(); e1.record(st)
    torch.cuda.synchronize()
    us = sorted(e0.elapsed_time(e1) * 1e3 for e0, e1 in ev)
    rounds.append(dict(best_us=round(us[0], 1), median_us=round(statistics.median(us), 1)))
print("QKV_TILE " + json.dumps(dict(label=label, lib=os.environ.get("SGL_LIB_PATH", "default"), tile=os.environ.get("SGL_NT_TILE", "default"),
                                    M=M, N=N, K=K, rounds=rounds, median_of_medians_us=statistics.median(r["median_us"] for r in rounds),
                                    tflops=round(2.0 * M * N * K / (min(r["best_us"] for r in rounds) * 1e-6) / 1e12, 1))), flush=True)
