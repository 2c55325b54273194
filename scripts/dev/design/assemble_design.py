import os
HERE=os.path.dirname(os.path.abspath(__file__))
ROOT=os.path.dirname(os.path.dirname(os.path.dirname(HERE)))
import json, re, sys
body=open(HERE+'/design_body.md').read()
tail=open(HERE+'/design_tail.md').read()
s0=open(HERE+'/design_s0.md').read()
s45=open(HERE+'/design_s45.md').read()
s7=open(HERE+'/design_s7.md').read()
def rep(a,b):
    global body
    assert body.count(a)==1, (body.count(a), a[:70])
    body=body.replace(a,b)
rep("replicated, host Cholesky (LU fallback) |", "replicated; Cholesky factor on every GPU, E⁻¹ = one device launch (section 4.5; host LU fallback) |")
rep("`E`, its factor: host, replicated.", "`E`: host, replicated; its Cholesky factor L and Lᵀ: on every GPU (2 dimE² doubles).")
rep("3. **E**: replicated and factored on the host (dimE ≤ a few thousand); `E⁻¹` costs one D2H/H2D of dimE\n   doubles per application.",
    "3. **E**: replicated and factored on the host (dimE ≤ a few thousand); since round 4 the factor is uploaded and `E⁻¹` is one\n   device launch per application (section 4.5; rounds 1–3: one D2H/H2D of dimE doubles and two host sweeps).")
rep("""The driver's CLI and its
`INFO:` / `TIME:` lines (§8 f1) are in `geneo4petsc_amd/driver.py`; lines 0, 1 and the solve line are
byte-identical to `tst/dummy/*.ref`, line 2 keeps the token layout `tst/plot.py` parses with this
build's solver names (`pcg-amg`, `lobpcg cholesky`), `tests/test_driver.py`.""", """The driver's CLI and its
`INFO:` / `TIME:` lines (§8 f1) exist twice: natively in C++ over the C ABI (`csrc/driver_main.cpp`, exported as
`GeneoDriverMain`, executable `geneo4petsc_amd/geneo_driver`: the readers of `--inpFileA` / `--inpFileB`, plugin loading, the
partitioner and decomposition calls, the PC, the output lines — round 4, north_star's "host code stays C++") and as the
Python prototype `geneo4petsc_amd/driver.py` it was ported from; `tests/test_driver.py` checks that the two print the same
`INFO:` lines character by character.  Lines 0, 1 and the solve line are byte-identical to `tst/dummy/*.ref`, line 2 keeps
the token layout `tst/plot.py` parses with this build's solver names (`pcg-amg`, `lobpcg cholesky`).""")
i2=body.index("**Fused LOBPCG update** (`k_lobpcg_update32`)")
body = body[:i2] + ("**Two-latency forms of the sliced SpMV kernels** (round 4: `row_sum_fixed`, `lp_row_sum_p16`).  A wave of the\n"
 "wave-per-slice kernels holds ONE 64-row slice, so its run time is a chain of dependent memory latencies, not bandwidth; the\n"
 "4-step loop sends a 7-wide slice through one round of four and three one-at-a-time tail steps — eight latencies ((col, val) →\n"
 "gather, four times).  For slices of at most 8 entries (FP64 SpMV) / 16 entries (companions: the 12-wide post-smoothing\n"
 "matrices) the body is instantiated per width: every (col, val) load first, then every gather, then the products in exactly\n"
 "the loop's order (KW / 4 rounds into four accumulators, the remainder into the first) — two latencies, bit-identical sums\n"
 "(`test_*_two_latency_form_is_bit_identical`).  A/B on one box, 6.5 M rows (`profiles/r04_two_latency_forms_ab.log`): companion passes\n"
 "89.5 → 79 µs, FP64 SpMV 117 → 110–114 µs, local solves −7 %.  The same sequence in the workgroup-per-slice companion kernel (each\n"
 "of four waves owning every fourth entry) costs what the narrow forms gain (92 against 82 µs) and is not built.\n\n") + body[i2:]
# insert 4.5 before section 5, and the round-4 tried-and-dropped paragraph
i=body.index("## 5. Oracle and parity")
dropped = ("**Tried and dropped in round 4**: *LDS window for the sliced SpMM* (VERDICT r3 item 2): per step group the wave loaded the\n"
 "U·RS + 2 rows next to its rows once, parked them in a wave-private LDS window and served every entry whose column fell inside\n"
 "it from there (per lane and entry, so correct for any pattern; 3 + 8 wave-wide loads per group instead of 14; bit-identical,\n"
 "tested).  126³ fine level, 32 columns: **0.481 ms with the window, 0.350 ms without** (`profiles/r04_spmm_lds_window_experiment.log`);\n"
 "in situ the class went from 0.475 to 0.586 ms per launch.  The window's load → LDS → read chain sits in front of the products\n"
 "of every group while the gathers it saves were the cheap ones (section 3: ± 1 rows cost 0.02 of the 0.33 ms).  *Two-latency\n"
 "form for the 12-wide post-smoothing matrices and the workgroup-per-slice companion kernels* (`lp_row_sum_p16`): kept (bit-identical,\n"
 "tested) although it moved the class by less than 1 % — those passes were not latency-chain bound (0.72 of the peak already);\n"
 "the 7-wide form is what moved it (84.0 → 80.1 µs at 6.5 M rows).  *Lanes-per-row kernel for the large ragged operators* (the\n"
 "0.86 M-row restriction and first coarse operator of a 6.5 M-row subdomain, `GENEO_SELL_VEC_MAX_ROWS` lifted): FP64 values instead\n"
 "of the companion's floats cost more than the better coalescing gains — solve 0.429 against 0.351 s\n"
 "(`profiles/r04_vec_kernel_for_large_ragged_ab.log`).\n\n")
body = body[:i] + dropped + s45.lstrip("\n") + "\n" + body[i:]
# section 5 additions
i=body.index("## 6. Multi-GPU")
par = ("**Round 4.**  (a) *Headline grids*: `tests/golden/headline.json` (`make_headline_goldens.py`; exact LU with a geometric\n"
 "nested-dissection ordering — `oracle._PermutedLU`, same factorisation as the default up to the elimination order, 25 PCG\n"
 "iterations at 64³ like the committed golden — and ARPACK shift-invert at 1e-3) holds the reference-literal oracle at the\n"
 "bench's argv on 96³ (@GOLD126@): PCG 24 for every operator perturbation 1e-14 … 1e-8 (not a threshold-hovering grid), GMRES 19\n"
 "(SRAS,1) and 11 (RAS,1), dimE 160, 20 vectors per subdomain.  `test_headline_grid_*`: GMRES counts identical, PCG within one\n"
 "of the oracle's spread, eigenvalues elementwise below the oracle's list (ARPACK at 1e-3 returns ONE 0.181798 where there are\n"
 "three) and equal up to the first missed copy; `bench.py` compares its own line with the golden of its grid\n"
 "(`golden_at_this_grid`).  (b) *48³* is declared with a band of 2: the last five residuals of the run are 7.0, 2.7, 4.5, 3.9,\n"
 "0.976 of the threshold (`profiles/r04_48cubed_shared_rho_counts.log`) — non-monotone by a factor 4 and under the threshold by\n"
 "2 % — so the count is 23 with one Gershgorin bound per level, 26 with one per subdomain, 25 at `-els2_eps_tol` 5e-4 and 2e-4\n"
 "either way (oracle 24; 22 with exact eigenvectors).  (c) *Converged solutions*: bench options at 24³, both Krylov loops at\n"
 "1e-13: library against oracle and against (1 … N), each within 1e-10 relative (measured 7e-14), CG and RAS + GMRES.\n"
 "(d) `-geneo_nicolaides_zero X` (1 = the reference's literal `min ≥ ε`, default 100): `test_nicolaides_zero_window_option`.\n\n")
body = body[:i] + par + body[i:]
# section 6: bench.py bullet
a=body[body.index("* **bench.py**: launched without torchrun"):body.index("* What grows with N at one subdomain per GPU")]
b=("* **bench.py**: launched without torchrun and `--gpus N > 1`, the parent touches no GPU, starts\n"
 "  `python -m torch.distributed.run --nproc-per-node N … bench.py …` as a child and relays its output.  `--scaling strong`\n"
 "  (default): the metric's 368³ grid in 2×2×2 subdomains at every N, block (bi, bj, bk) on the rank whose box of the rank grid\n"
 "  (1×1×1, 2×1×1, 2×2×1, 2×2×2) holds it — 8 / 4 / 2 / 1 subdomains per GPU; ranks holding several subdomains eigensolve them\n"
 "  group by group (section 4.5; gloo world-size-2 test with four subdomains per rank and one per group).  `--scaling weak`:\n"
 "  the round-1..3 lines (126³ in 8 subdomains at N = 1, 184³ and one subdomain per GPU at N > 1).  The host-side\n"
 "  decomposition is windowed (`decompose_grid_domain`: each rank touches only box ⊕ (2·overlap+3) nodes), the rank's\n"
 "  subdomains are built side by side on host threads, and the halo plan is computed locally (`grid_rank_plan`).  One PC\n"
 "  object is set up again for every step.\n")
body=body.replace(a,b)
nums=json.load(open(HERE+'/design_nums.json')) if len(sys.argv)>1 else {}
out = s0 + "\n" + body.rstrip("\n") + "\n\n" + s7 + "\n" + tail
for k,v in nums.items():
    out=out.replace("@%s@"%k, str(v))
left=sorted(set(re.findall(r"@[A-Z0-9]+@", out)))
open(ROOT+'/DESIGN.md' if len(sys.argv)>1 else HERE+'/DESIGN_preview.md','w').write(out)
print("lines", len(out.split("\n")), "unfilled", left)
