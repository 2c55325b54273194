// GenEO preconditioner core (host orchestration over the device primitives of backend.h).
// MI355X-native counterpart of /root/reference/src/geneo.cpp; see DESIGN.md for the map.
#pragma once
#include <cstdint>
#include <future>
#include <memory>
#include <string>
#include <map>
#include <vector>

#include "backend.h"

namespace geneo {
class AmgDevice;

struct HostCsr {
  int n = 0;
  std::vector<int> rowptr, col;
  std::vector<double> val;
  bool empty() const { return rowptr.empty(); }
};

// -geneo_* options: names, defaults and validation follow geneo.cpp:2329-2514 / :2649-2662.
struct Options {
  bool lvl1ASM = true, lvl1RAS = false, lvl1SRAS = false, lvl1ORAS = false;
  int lvl2 = 1;
  bool hybrid = false, effHybrid = false;
  double optim = 0.0, tau = 0.1, gamma = 10.0;
  bool cst = false;
  int cut = -1;
  bool noSyl = false, offload = false;
  bool check = false;      // -geneo_chk (geneo.cpp:2466-2479)
  // -geneo_nicolaides_zero <x>: the Nicolaides rule (geneo.cpp:896-944) takes min(lambda) >= x DBL_EPSILON as "zero has
  // not been found".  1 = the reference's literal test; default 100 (a computed zero eigenvalue of an exactly singular
  // Neumann matrix is a rounding error of either sign around 1e-16 .. 2e-15: core.cpp)
  double nicolaides_zero = 100.0;
  // -els2_ : local eigensolver (LOBPCG on the GPU replaces ARPACK shift-invert, geneo.cpp:626-744)
  double eps_tol = 1e-3;   // EPSSetTolerances default at geneo.cpp:658
  int eps_nev = 16;        // block target when -geneo_cut is not given (no inertia count on the GPU)
  int eps_max_it = 500;
  int eps_block = 0;       // LOBPCG block size m (0 = auto: multiple of 16 >= nev + guard)
  std::string eps_conv = "sinvert";   // convergence test: ARPACK's shift-invert Ritz estimate | plain "residual" (core.cpp)
  int cheb_degree = 6;     // Chebyshev-Jacobi preconditioner inside LOBPCG
  double cheb_ratio = 20.0;
  double rr_drop = 1e-6;   // pivot threshold of the rank-revealing Rayleigh-Ritz (basis conditioning <= 1/drop)
  uint64_t eps_seed = 0;
  // Memory-bounded set-up (-geneo_eig_group_rows / -geneo_eig_mem_gb): LOBPCG carries ~30 m doubles per local row (m = block
  // width; 7.7 KB per row at m = 32) next to the A_Neu hierarchy -- eight 6.5 M-row subdomains of the 368^3 benchmark on
  // ONE GPU would need 400 GB.  When the rank's subdomains exceed the budget they are eigensolved in consecutive groups
  // (each group: its own fine matrices, A_Neu hierarchy and basis blocks, released before the next one starts); the
  // per-subdomain iteration is independent of its neighbours in the batch, so the eigenpairs are the ungrouped ones.
  //   eig_group_rows > 0: at most this many local rows per group (a subdomain is never split);  0: from the budget
  //   eig_mem_gb     > 0: device-memory budget of one group's eigensolve in GiB;  0: 35 % of the card (unknown card: one group)
  int eig_group_rows = 0;
  double eig_mem_gb = 0.0;
  // Coarse start of the local eigensolves (-geneo_eig_coarse_start R): when every subdomain of the batch (the rank's
  // subdomains, or one group of the memory-bounded set-up) holds at least R rows, LOBPCG first runs on the Galerkin pencil of multigrid level 1 (A_c = P^T A_Neu P from the hierarchy,
  // B_c = P^T D A_Dir D P: two sparse products) and the fine iteration starts from the prolonged Ritz vectors instead of a
  // random block: an iteration there costs an eighth of a fine one and the fine solve is left with the last digits.  The
  // fine pairs meet the same convergence test either way.  0: never.
  int eig_coarse_start = 750000;
  // -dls1_ : local "direct" solve replaced by batched Jacobi-PCG driven to a tight tolerance
  double dls1_rtol = 1e-12;
  int dls1_max_it = 20000;
  int dls1_check = 16;     // host convergence poll period (iterations; 4 with the AMG preconditioner)
  // -dls1_ksp_type cg|chebyshev: the batched V-cycle-PCG above, or a fixed-degree Chebyshev iteration preconditioned by
  // the same V-cycle (needs -dls1_pc_type amg): no reductions, no host polling, a fixed linear operator p(VA)V at any
  // -dls1_ksp_rtol.  Per subdomain: eigenvalue bounds of VA from -dls1_cheb_esteig_its Lanczos steps, scaled by
  // -dls1_cheb_safety lo,hi; the degree is the smallest k with 1 / T_k(sigma) <= -dls1_ksp_rtol (at most -dls1_ksp_max_it).
  std::string dls1_ksp = "cg";
  int dls1_cheb_esteig_its = 16;
  double dls1_cheb_safety_lo = 0.9, dls1_cheb_safety_hi = 1.1;
  // inner preconditioners: "amg" = smoothed-aggregation V-cycle (default), "jacobi" / "cheb" = round-1 baseline
  std::string dls1_pc = "amg", els2_pc = "amg";
  int amg_coarse_size = 600, amg_smooth_degree = 1, amg_max_levels = 10;
  double amg_smooth_ratio = 4.0;
  // the same per hierarchy (0: the common -amg_smooth_ratio): -dls1_amg_smooth_ratio for the level-1 hierarchy of the local
  // solves, -els2_amg_smooth_ratio for LOBPCG's A_Neu hierarchy
  // Local solves: 12 -- the damped-Jacobi weight 1 / (0.55 rho (1 + 1 / ratio)) grows from 1.45 / rho (ratio 4) to 1.68 / rho
  // against a Gershgorin bound that overestimates rho(D^-1 A): one rank of 368^3, 496 -> 440 inner iterations, solve 0.391 ->
  // 0.349 s, flat from 12 up (profiles/r04_inner_solver_sweep_rank_of_8.log).  The inner PCG runs to -dls1_ksp_rtol whatever
  // its preconditioner, so the outer iteration is unchanged.  LOBPCG's hierarchy keeps 4: its V-cycle is also the ruler of
  // the convergence test at -els2_eps_tol (8: 19 -> 18 iterations, and a different ruler).
  double dls1_amg_smooth_ratio = 12.0, els2_amg_smooth_ratio = 0.0;
  // -dls1_amg_strength / -els2_amg_strength (AmgParams::strength).  Local solves: 0.04 (126^3: 26 -> 18 inner iterations per
  // solve, same outer counts).  LOBPCG's hierarchy keeps every connection: its V-cycle is also the ruler of the convergence
  // test at -els2_eps_tol, and a different ruler moves the outer iteration count at the loose tolerance of the benchmark
  // (126^3: 25 -> 23) away from the reference-literal oracle's.
  double dls1_amg_strength = 0.04, els2_amg_strength = 0.0;
  // -geneo_coarse_device auto|never|always: where the replicated coarse operator E is factored and solved.
  //   never:  host Cholesky (LU when that fails); sweeps in one workgroup up to dimE 1024, on the host above
  //   auto:   as never up to dimE 1024; above: blocked device factorisation and blocked device sweeps (coarse_dev.h)
  //   always: the blocked device kernels at any dimE > 0
  // Whenever the device factorisation is not to be had (backend without the kernels, E not positive definite to rounding,
  // no device memory) the host sequence runs instead, with the host round trip in the apply.
  // -geneo_coarse_block nb: block size of those kernels, a multiple of 16 in 16 .. 256
  enum CoarseDevice { COARSE_AUTO = 0, COARSE_NEVER = 1, COARSE_ALWAYS = 2 };
  int coarse_device = COARSE_AUTO;
  int coarse_block = 128;   // within 7 % of the best sweeps and 1.5 x of the best factor time at 1256 .. 5120
  // -geneo_block_width 0|16|32: slab width of the block entry points (PCMatApply_GenEO, MatMatMult_GenEO,
  // KSPMatSolve_GenEO).  0: none -- the set-up allocates and builds nothing for them.  16 | 32: needs -dls1_ksp_type
  // chebyshev (a fixed linear operator: the block local solve is its chain of launches with SpMM in place of SpMV).  Read
  // by the set-up: a change afterwards has no effect before the next set-up.
  int block_width = 0;
  bool dls1_amg_single = true;   // -dls1_amg_precision single|double: storage of the level matrices the V-cycle of the local solves reads
  // Krylov driver (counterpart of the PETSc KSP the reference calls at driver:1240)
  std::string ksp_type = "gmres";
  // -ksp_matsolve_type cg|gmres: the Krylov method of KSPMatSolve_GenEO alone; unset (empty): -ksp_type, which must be cg
  std::string ksp_matsolve_type;
  // -ksp_pc_side left|right (unset, empty: left).  right with -ksp_type gmres: right-preconditioned GMRES; -ksp_type fgmres
  // is always right (flexible GMRES: the preconditioner may change from step to step); cg is left only
  std::string ksp_pc_side;
  bool right_side() const { return ksp_type == "fgmres" || ksp_pc_side == "right"; }
  // -ksp_type fcg (flexible CG, left-preconditioned): -ksp_fcg_mmax m >= 1 directions a new one is made conjugate to,
  // -ksp_fcg_truncation_type notay|standard (csrc/fcg_window.h), -ksp_norm_type preconditioned|unpreconditioned (unset,
  // empty: preconditioned; unpreconditioned is fcg's alone: the test is on |b - A x|, which its step returns)
  int ksp_fcg_mmax = 30;
  bool ksp_fcg_mmax_set = false;
  std::string ksp_fcg_truncation;    // unset (empty): notay
  std::string ksp_norm_type;
  double ksp_rtol = 1e-5, ksp_atol = 1e-50, ksp_dtol = 1e5;
  int ksp_max_it = 10000, ksp_restart = 30;
  bool ksp_guess_nonzero = true;   // driver:1348 always sets it
  std::string name() const;        // buildGenEOName, geneo.cpp:2245-2268
};
// returns "" on success, otherwise the error message (same texts as the reference)
std::string parse_option(Options& o, const std::string& key, const std::string& value);
std::string validate_options(const Options& o);
// validation switches: "cheb_fused" 1 (default) bk::cheb_dir and bk::cheb_residual, 0 the same step and residual update
// composed of backend.h primitives (gather, block_colscale, axpy, block_rowscale, copy; spmv, axpy); "block_fused" 1
// (default) the kernels of block_dev.h, 0 the same operations composed of backend.h primitives (the definitions the host
// twin links)
void set_cheb_fused(int on);
int cheb_fused();
void set_block_fused(int on);
int block_fused();
// "krylov_fused" 1 (default) the kernels of krylov_dev.h, 0 their composed forms (one bk::dot / bk::axpy per basis vector)
void set_krylov_fused(int on);
int krylov_fused();
struct StepWork {   // scratch of the composed step at width w: one slab, the coefficients spread over the columns, their gather indices
  double *t = nullptr, *ab = nullptr;
  int* idx = nullptr;
  int n = 0, ns = 0, w = 0;
  void alloc(int n, int ns, int w);
  void release();
};
// core.cpp: the arithmetic of bk::cheb_dir (w = 1) / bk::cheb_dir_block from backend.h primitives, on the caller's scratch;
// the _once forms allocate their scratch, run, wait, free
bool cheb_dir_composed(const bk::Chunks& c, const double* coef_k, int flags, const double* Z, double* D, double* X,
                       const double* dscale, double* Out, int w, const StepWork& wk);
bool cheb_dir_composed_once(const bk::Chunks& c, const double* coef_k, int flags, const double* Z, double* D, double* X,
                            const double* dscale, double* Out, int w);
bool block_import_composed(const double* Xcm, int ld, int n, int m, double* Yrm, int w);
bool block_export_composed(const double* Xrm, int w, int n, int m, double* Ycm, int ld);
bool block_coldot_composed_once(const double* X, const double* Y, int n, int w, double* out);
bool block_axpy_cols_composed_once(double* Y, const double* X, const double* c, int n, int w);
bool block_xpby_cols_composed_once(double* P, const double* Z, const double* c, int n, int w);
bool chol_solve_block_composed_once(const double* L, const double* LT, int n, double* Y, int w);
// the Gram-Schmidt passes of the block GMRES, one bk::block_coldot / bk::block_axpy_cols per basis slab (Vh: slab pointers
// on the host); the _once forms read the pointer table from the device, as bk::block_gs_dots / _update do, and wait
bool block_gs_dots_composed(const double* const* Vh, int nb, const double* W, int n, int w, double* H, double* work);
bool block_gs_update_composed(double* Y, const double* const* Vh, int nb, const double* C, int n, int w, double* norm2,
                              double* work);
bool block_gs_dots_composed_once(const double* const* V, int nb, const double* W, int n, int w, double* H, double* work);
bool block_gs_update_composed_once(double* Y, const double* const* V, int nb, const double* C, int n, int w, double* norm2,
                                   double* work);
bool block_scale_cols_composed_once(double* Out, const double* X, const double* c, int n, int w);
// the Gram-Schmidt passes of the right-preconditioned GMRES (krylov_dev.h) from bk::dot and bk::axpy, one call per basis
// vector (Vh: the vector pointers, Ch: the coefficients, both on the HOST); the _once forms read the pointer table and the
// coefficients from the device, as bk::vec_gs_dots / bk::vec_gs_update do, and wait
bool vec_gs_dots_composed(const double* const* Vh, int nb, const double* W, int n, double* H);
bool vec_gs_update_composed(double* Y, const double* const* Vh, int nb, const double* Ch, int n, double* norm2);
bool vec_gs_dots_composed_once(const double* const* V, int nb, const double* W, int n, double* H);
bool vec_gs_update_composed_once(double* Y, const double* const* V, int nb, const double* C, int n, double* norm2);
// bk::vec_fcg_step from backend.h primitives: S ([eta, pi], on the device) is downloaded, then bk::axpy, bk::axpy, bk::dot
bool vec_fcg_step_composed(double* x, double* r, const double* p, const double* w, const double* S, int n, double* norm2);

struct Info {                 // public counters / timers of geneoContext (hdr/geneo.hpp:96-123)
  int estimDimELoc = 0, realDimELoc = 0, nicolaidesLoc = 0, dimE = 0;
  int eig_iterations = 0, eig_spmm = 0;
  long long dls1_iterations = 0, dls1_solves = 0;
  double lvl1SetupMinvTimeLoc = 0, lvl2SetupEigTimeLoc = 0, lvl2SetupZTimeLoc = 0, lvl2SetupETimeLoc = 0;
  double lvl1ApplyTimeLoc = 0, lvl1ApplyScatterTimeLoc = 0, lvl1ApplyMinvTimeLoc = 0, lvl1ApplyGatherTimeLoc = 0;
  double lvl1ApplyPrjFSTimeLoc = 0, lvl2ApplyTimeLoc = 0, lvl2ApplyZtTimeLoc = 0, lvl2ApplyEinvTimeLoc = 0,
         lvl2ApplyZTimeLoc = 0;
  double setupTime = 0, solveTime = 0;
  long long spmv_calls = 0;
  int amg_levels = 0, amg_on_device = 0;
  int eig_groups = 1;          // consecutive subdomain groups the eigensolve ran in (memory-bounded set-up)
  int eig_coarse_iterations = 0;   // LOBPCG iterations on the multigrid level-1 pencil (coarse start; 0: not used)
  double amg_operator_complexity = 0.0, amgSetupTime = 0.0;
  int nullPivotsLoc = 0;
};

struct KspResult {
  int its = 0;
  double rnorm = 0.0;
  int reason = 0;     // PETSc KSPConvergedReason numbering (2 RTOL, 3 ATOL, -3 ITS, -4 DTOL, -9 NANORINF ...)
};

typedef int (*exchange_fn)(void* user, int reverse);
typedef int (*allreduce_fn)(void* user, int n);

class PC {
 public:
  Options opt;
  Info info;
  std::string last_error;

  // ---- inputs (initGenEOPC / PCGenEOSetup, geneo.cpp:2518-2632) ----------------------------
  int N = 0;                 // nbDOF
  int nsub_global = 0;
  int rank = 0, size = 1;
  std::vector<int> owned;    // ascending global ids owned by this rank (all of 0..N-1 when size==1)
  struct Sub {
    int gid = 0;             // global subdomain id (= MPI rank in the reference)
    std::vector<int> l2g;    // dofIdxDomLoc (ascending global ids)
    std::vector<int> mult;   // dofIdxMultLoc
    HostCsr a_neu, a_dir;    // MATIS local matrix / optional pcADirLoc
    std::vector<char> intersect;  // intersectLoc emptiness per global subdomain (GenEO-2 gamma_loc only)
  };
  std::vector<Sub> subs;
  // halo plan (size > 1)
  std::vector<int> halo_gid, recv_counts, send_counts, send_idx;
  exchange_fn cb_exchange = nullptr;
  allreduce_fn cb_allreduce = nullptr;
  void* cb_user = nullptr;
  double *comm_send = nullptr, *comm_recv = nullptr, *comm_red = nullptr;  // device buffers owned by the caller
  int comm_red_cap = 0;
  int comm_width = 1;        // the halo buffers hold this many vectors per exchange (PCGenEOSetCommWidth)

  PC();
  ~PC();
  int add_subdomain(int gid, int n, const int* l2g, const int* mult, const int* neu_rowptr, const int* neu_col,
                    const double* neu_val, const int* dir_rowptr, const int* dir_col, const double* dir_val);
  int set_intersect(int gid, int nb, const int* nonempty);   // intersectLoc of initGenEOPC (hdr/geneo.hpp:34)
  int setup(const double* b_dev);                       // setUpGenEOPC, geneo.cpp:1672
  int apply(const double* x_dev, double* y_dev);        // applyGenEOPC, geneo.cpp:2051
  int apply_q(const double* x_dev, double* y_dev);      // applyQ, geneo.cpp:1435
  // where E was factored and how E^-1 is applied (PCGenEOGetCoarseInfo)
  void coarse_info(int* dim, int* factor_on_device, int* solve_kind, int* block) const;
  // Chebyshev local solver (-dls1_ksp_type chebyshev), per local subdomain: the bounds [lo, hi] of the V-cycle-
  // preconditioned operator, the degree k_s and ||r_K|| / ||b|| of the verification solve of the set-up (empty: cg path)
  std::vector<double> cheb_lo, cheb_hi, cheb_achieved;
  std::vector<int> cheb_its;
  int matmult(const double* x_dev, double* y_dev);      // MatMult(MATIS)
  int solve(const double* b_dev, double* x_dev, KspResult* res);  // KSPSolve counterpart
  // ---- blocks of right-hand sides (-geneo_block_width 16 | 32): column-major n_owned x m blocks with a leading dimension,
  // processed in slabs of the width (the last one zero-padded).  Each returns an error for a set-up without a width.
  int apply_mat(const double* X, int ldx, double* Y, int ldy, int m);        // PCMatApply: Y = M^-1 X
  int matmult_mat(const double* X, int ldx, double* Y, int ldy, int m);      // MatMatMult: Y = A X
  // KSPMatSolve: PCG (or, -ksp_matsolve_type gmres, restarted GMRES) on every column in lock step, zero initial guess (X is
  // zeroed here); its / rnorm / reason: m entries
  int solve_mat(const double* B, int ldb, double* X, int ldx, int m, int* its, double* rnorm, int* reason);
  // since the set-up: slabs applied by apply_mat (KSPMatSolve's included), their columns, the zero columns that padded
  // them, and the local solves of slabs replayed from the HIP graph (the others went out as direct launches)
  void block_info(int* width, long long* slabs, long long* columns, long long* padded, long long* graph_launches) const;
  // block GMRES (PCGenEOGetBlockKrylovInfo): basis slabs held and the bytes of the basis with its tables and partial sums
  // (0 before the first block GMRES solve of a set-up), and since the set-up the Gram-Schmidt passes that went through
  // bk::block_gs_dots / bk::block_gs_update and through their composed forms
  void block_krylov_info(int* basis_slabs, double* basis_bytes, long long* gs_fused, long long* gs_composed) const;
  // right-preconditioned / flexible GMRES (PCGenEOGetKrylovInfo): device vectors held now (basis V, the flexible basis Z
  // and the scratch vectors) and their bytes with the tables, coefficients and partial sums (0 before the first such solve
  // of a set-up); since the set-up the Gram-Schmidt passes through bk::vec_gs_dots / bk::vec_gs_update and through their
  // composed forms; and the preconditioner applications and operator products of the last solve()
  void krylov_info(int* basis_vectors, double* basis_bytes, long long* gs_fused, long long* gs_composed, long long* pc_applies,
                   long long* mat_mults) const;
  // since the set-up: slab applications of E^-1 by the blocked block sweeps (bk::coarse_solve_block), column by column
  // through the single-vector path, and by one host round trip of the whole block (PCGenEOGetCoarseBlockCounters)
  void coarse_block_counters(long long* blocked, long long* by_column, long long* host_blocks) const;
  // flexible CG (PCGenEOGetFcgInfo): direction / product pairs held now and the device bytes of everything the method
  // holds (0 before the first fcg solve of a set-up); since the set-up the steps through bk::vec_fcg_step and through its
  // composed form; of the last fcg solve the largest window and the downloads (device-to-host copies the host waited for)
  void fcg_info(int* directions, double* bytes, long long* steps_fused, long long* steps_composed, int* max_window,
                long long* downloads) const;
  int n_owned() const { return (int)owned.size(); }
  int cheb_steps_per_solve() const { return cheb_K; }
  void cheb_counters(long long* solves, long long* graph_launches, long long* fused_residuals) const {
    *solves = cheb_chain.runs;
    *graph_launches = cheb_chain.replays;
    *fused_residuals = cheb_res_fused;
  }
  std::vector<double> cheb_table() const;   // the device coefficient table, K x nsub x 2 (download)
  const double* x0_dev() const { return d_x0; }
  // results for parity tests
  std::vector<std::vector<double>> eigvals;      // per local subdomain: eigenvalues kept in Z
  std::vector<std::vector<double>> candidates;   // per local subdomain: all converged Ritz values
  std::vector<double> E;                         // dimE x dimE (row-major)
  std::vector<int> ksub_global;                  // realDimE per global subdomain
  std::vector<double> residual_history;
  std::vector<double> tauLoc, gammaLoc;          // per local subdomain (GenEO-2, geneo.cpp:1097-1232)

 private:
  bool is_setup = false;
  int nL = 0, nE = 0, nH = 0;        // local space, ext (= owned + halo), halo sizes
  std::vector<int> suboff;
  bk::Chunks ch;
  bk::Csr neuL, neuE, dirL;          // block-diagonal CSRs (neuE shares rowptr/val with neuL)
  int *d_l2e = nullptr, *d_rt_ptr = nullptr, *d_rt_idx = nullptr, *d_send_idx = nullptr;
  int *d_rv_ptr = nullptr, *d_rv_idx = nullptr, *d_rv_tgt = nullptr;
  int n_rv = 0;
  double *d_D = nullptr, *d_dinv1 = nullptr, *d_dinvN = nullptr;
  double *d_xe = nullptr, *d_ye = nullptr, *d_xL = nullptr, *d_wL = nullptr;
  double *d_cg_r = nullptr, *d_cg_z = nullptr, *d_cg_p = nullptr, *d_cg_q = nullptr, *d_cg_sc = nullptr;
  double *d_t1 = nullptr, *d_t2 = nullptr, *d_t3 = nullptr, *d_x0 = nullptr, *d_scal = nullptr;
  double *d_rvtmp = nullptr;
  // coarse space
  double* d_Z = nullptr;
  int64_t* d_zbase = nullptr;
  int *d_ksub = nullptr, *d_zoff = nullptr, *d_subgid = nullptr;
  std::vector<int> ksub, zoff;
  int kmax = 0, dimE = 0;
  double* d_yE = nullptr;
  double *d_EL = nullptr, *d_ELT = nullptr;   // Cholesky factor of E and its transpose on the device (coarse_solve_local)
  std::vector<double> Efac, EfacT;
  std::vector<int> Epiv;
  bool E_chol = true;
  bool E_dev = false;     // d_EL / d_ELT were factored on the device (block size E_nb): blocked sweeps in coarse_solve_local
  int E_nb = 0;
  bool factor_E_on_device(const std::vector<double>& sym);
  std::vector<double> h_yE, h_yEblk;   // host staging of one coarse vector / of a dimE x w block (coarse_einv)
  std::vector<double> h_Dscratch;   // partition of unity on the host, reused by the next set-up
  double cheb_lmax = 2.0, cheb_lmax1 = 2.0;
  struct Amg1Pending;
  std::unique_ptr<Amg1Pending> pend1;   // level-1 hierarchy whose host set-up is still running
  int finish_amg1();
  bool eig_only = false;       // a group's temporary PC (eigen_grouped): the set-up stops behind the eigensolve
  std::vector<int> eig_groups; // boundaries of the subdomain groups of this set-up ({0, ns}: one group = the plain path)
  double prepare_secs = 0.0;   // time of setup_prepare (setupTime = both halves)
  double release_secs = 0.0;   // time setup_prepare spent releasing the previous set-up (outside setupTime)
  std::promise<bool>* subs_released = nullptr;   // PC::setup's overlapped mode: fulfilled once setup_prepare no longer reads `subs`
  bool eig_early = false;      // the eigensolves of this set-up have run already (overlapped mode)
  void fill_partition_of_unity();
  int setup_level2_eigen();
  int setup_prepare();         // first half of setup(): everything the eigensolve waits for
  int setup_finish(const double* b_dev);   // second half: level 2 and the bookkeeping
  std::vector<int> plan_eig_groups() const;
  int eigen_grouped();
  std::map<int, void*> cg_graphs;   // HIP graphs of an inner-PCG chunk, by 2 * chunk length + rz parity at its start (local_solve)
  int cg_long_len = 0;         // length of the first chunk of a local solve once the first solve of this set-up is known (0: not yet, -1: never)
  bool cg_graph_failed = false;
  long long cg_chunks = 0;     // chunks issued so far (sampling of direct launches while the in-situ timer runs)
  // A chain of launches captured once into a HIP graph and replayed (the Chebyshev local solve, one per width)
  struct Replay {
    void* graph = nullptr;
    bool failed = false;
    const void* buf = nullptr;          // what the graph was captured for: the buffer it names and the *_fused value
    int fused = -1;                     // (recaptured when either changes)
    long long runs = 0, replays = 0;    // runs so far, and those that replayed the graph (the others: direct launches)
    int value = 0;                      // what the chain returned when it was recorded
    template <class Body>
    int run(const void* buf, int fused, Body&& body);   // the value of this run's chain
    void reset();
  };
  // What an application of the preconditioner works on.  Two instances, filled by the set-up: `vec` (w = 1, always) and
  // `slab` (w = -geneo_block_width, row-major slabs; w = 0 without one).  The slab path is the vector path at another width:
  // restrict / prolong / matmult / cheb_steps / apply_on / apply_q_on take the width from here, and only local_solve and
  // the coarse_* leaves branch on w == 1.
  struct App {
    int w = 0;
    bool coarse = false;                 // Q is applied (slab: a non-empty coarse space; vec: its kernels take dimE = 0)
    double *wl = nullptr, *xl = nullptr; // local: right-hand side -> result of the local solve; R x of apply_q = the chain's solution
    double *r1 = nullptr, *z = nullptr, *d = nullptr;   // local, the chain's: second residual (ping-pong), V r, direction
    double *t1 = nullptr, *t2 = nullptr, *t3 = nullptr; // owned temporaries of the generic composition
    double *xe = nullptr, *ye = nullptr; // ext staging of the restriction / the prolongation
    StepWork* work = nullptr;            // scratch of the composed step
    Replay* chain = nullptr;
  };
  App vec, slab;
  // Chebyshev local solver: coefficient table coef[(k ns + s) 2 + {0, 1}] = (a_k, b_k) of subdomain s (rows k >= k_s are
  // zero), K = max_s k_s steps per solve, and per width the HIP graph of one whole solve with its counters
  // (PCGenEOGetLocalSolverCounters, PCGenEOGetBlockInfo) and the scratch of the composed step (vector: sized by setup_cheb;
  // slab: by the first composed solve).  cheb_res_fused: residual updates r - A d of vector solves that went through
  // bk::cheb_residual (the others: bk::spmv and bk::axpy).
  double* d_cheb_coef = nullptr;
  int cheb_K = 0;
  long long cheb_res_fused = 0;
  Replay cheb_chain, blk_chain;
  StepWork cheb_work, blk_work;
  int setup_cheb();
  void cheb_release();
  int cheb_steps(const App& a, const double* dscale);   // returns the number of residual updates bk::cheb_residual took
  // Block entry points: slab width of this set-up (0: none), the work space (local slabs r -- two, ping-pong --, z, d, x;
  // owned slabs in / out / t1..t3; the ext staging slab; coarse right-hand sides, per-subdomain Gram rows and
  // coefficients), the row-major Z, the index maps between Gram rows, coarse rows and coefficient rows, and the counters
  // of PCGenEOGetBlockInfo
  int blk_w = 0, blk_kp = 0;
  double *blk_r0 = nullptr, *blk_r1 = nullptr, *blk_z = nullptr, *blk_d = nullptr, *blk_x = nullptr;
  double *blk_in = nullptr, *blk_out = nullptr, *blk_t1 = nullptr, *blk_t2 = nullptr, *blk_t3 = nullptr, *blk_xe = nullptr;
  double *blk_yE = nullptr, *blk_G = nullptr, *blk_C = nullptr, *blk_ZR = nullptr, *blk_col = nullptr;
  double *blk_dots = nullptr, *blk_dotwork = nullptr, *blk_coef = nullptr;
  int *blk_g2e = nullptr, *blk_e2c = nullptr;
  long long blk_slabs = 0, blk_columns = 0, blk_padded = 0;
  long long coarse_blk_blocked = 0, coarse_blk_by_column = 0, coarse_blk_host = 0;   // coarse_block_counters
  int setup_block();
  void block_release();
  int block_check(const char* who, int ld, int m, const void* a, const void* b);
  int slab_loop(bool apply, const double* X, int ldx, double* Y, int ldy, int m);   // apply_mat / matmult_mat
  void slab_in(const double* Xcm, int ld, int m, double* slab);
  void slab_out(const double* slab, int m, double* Ycm, int ld);
  void slab_coldot(const double* X, const double* Y, double* h_out);
  void slab_cols(bool xpby, double* A, const double* B, const double* h_c);
  int solve_cg_block(const double* B, int ldb, double* X, int ldx, int m, int* its, double* rnorm, int* reason);
  // block GMRES: the basis slabs with their device pointer table, dots / coefficients (slabs x w each) and the partial sums
  // of bk::block_gs_dots; allocated by the first block GMRES solve, grown as the steps need them, freed by block_release
  std::vector<double*> blk_basis;
  double** blk_basis_tab = nullptr;
  double *blk_gs_h = nullptr, *blk_gs_c = nullptr, *blk_gs_work = nullptr;
  double blk_gs_bytes = 0.0;
  long long blk_gs_fused = 0, blk_gs_composed = 0;
  void basis_grow(int slabs);
  int solve_gmres_block(const double* B, int ldb, double* X, int ldx, int m, int* its, double* rnorm, int* reason);
  HostCsr host_neu_cache, host_dir_cache;   // block-diagonal host copies of A_Neu / the level-1 matrix, reused by the next set-up
  AmgDevice* amg1 = nullptr;   // hierarchy of the level-1 (Dirichlet / Robin) block-diagonal matrix (local solves)
  AmgDevice* amgN = nullptr;   // hierarchy of the Neumann block-diagonal matrix (LOBPCG preconditioner)

  int fail(const std::string& msg);
  int build_layout();
  int ensure_dirichlet();
  void make_robin(Sub& s, HostCsr& out) const;
  int setup_level2(const double* b_dev);
  struct EigProblem {
    const bk::Csr* A; const double* As;   // Y = As .* A (As .* X); As may be null
    const bk::Csr* B; const double* Bs;
    AmgDevice* amg;                       // V-cycle of A as preconditioner (null: Chebyshev-Jacobi)
    const double* dinv; double lmax;      // Jacobi scaling and Gershgorin bound for the Chebyshev fallback
    int nev_try;
    const char* label;
    // deflated restart (no -geneo_cut and more eigenvalues below the threshold than one block holds): the iteration runs
    // in the B-orthogonal complement of the locked blocks Y_b (n_L x k_b row-major, B-orthonormal per subdomain, zero
    // columns where a subdomain locked fewer), BY_b = B Y_b; subdomains with skip[s] != 0 are frozen from the start
    struct Locked { const double* Y; const double* BY; int k; };
    const std::vector<Locked>* defl = nullptr;
    const char* skip = nullptr;
    const int* locked_cols = nullptr;     // per subdomain: columns locked so far (bounds the pairs that can still be asked for)
    int seed_off = 0;
    double tol = 0.0;                     // > 0: convergence tolerance of this solve instead of -els2_eps_tol
    // A and B on ONE sliced pattern (bk::spmm_dual): A W and B W of an iteration in one pass over W
    const bk::Csr* dual_pat = nullptr;
    const double *dual_vA = nullptr, *dual_vB = nullptr;
    // A pencil that does not live on the fine rows (the coarse start of eigen_lobpcg: the Galerkin pencil of multigrid
    // level `amg_level`): its row count, the chunks of its subdomain blocks and the blocks' row offsets (ns + 1)
    int rows = -1;
    const bk::Chunks* chunks = nullptr;
    const int* row_off = nullptr;
    int amg_level = 0;                    // the V-cycle starts at this level of `amg`
    const double* X0 = nullptr;           // start block (rows x m row-major, device) instead of the seeded random one
    int* iterations = nullptr;            // where the iteration count goes (default: info.eig_iterations)
    int max_it = 0;                       // > 0: at most this many iterations, and the block is handed back as it stands then
                                          // (a start block for the next level does not have to meet the tolerance)
  };
  int lobpcg_solve(const EigProblem& P, int m, std::vector<double>& lam, double* Xc);
  int eig_targets(int* nev_try) const;
  int eig_block_max() const;
  void local_tau();
  int local_gamma();
  int check_global_spd();
  int check_local_spd(const EigProblem& P, const HostCsr* const* hostB, bool scale_mult);
  int check_local_rank();
  int check_global_rank();
  int eigen_dense_host();
  int eigen_lobpcg();
  int build_E();
  // R (applyLevel1Scatter), sum R^T (applyLevel1Gather) and A = sum R^T A_Neu R on w vectors (w > 1: row-major); at
  // w > 1 the halo buffers hold w x the single-vector counts and the exchange callback gets flag = reverse | w << 1
  void restrict(const double* X, double* XL, int w, double* xe);
  void prolong(const double* WL, double* Y, int w, double* ye);
  void matmult(const double* X, double* Y, int w, double* WL, double* xe, double* ye);
  void local_solve_cg(double* wL);                                // [D] M^-1 [D]: batched PCG (vector only)
  void local_solve(const App& a);                                 // [D] M^-1 [D] on a.wl: PCG (w = 1) or the Chebyshev chain
  void coarse_einv(double* yE, int w);                            // yE <- E^-1 yE (the factor's own path)
  void coarse_solve(const App& a, const double* XL);              // coarse coefficients E^-1 Z^T x (from the restricted XL)
  void coarse_expand(const App& a, double* WL, bool add);         // WL (+)= Z times those coefficients
  void apply_q_on(const App& a, const double* X, double* Y);
  void apply_on(const App& a, const double* X, double* Y);
  void allreduce(double* dev, int n);
  double gdot(const double* x, const double* y);
  int solve_cg(const double* b, double* x, KspResult* res);
  int solve_gmres(const double* b, double* x, KspResult* res);
  // Right-preconditioned (flexible: Z_k = M^-1 v_k is kept) GMRES.  Its memory -- basis vectors V and Z, scratch vectors,
  // the device pointer tables, coefficient slots and the partial sums of bk::vec_gs_dots -- is allocated by the first such
  // solve, grown as the steps need it, kept for the next solve and freed by krylov_release (with the set-up)
  std::vector<double*> kr_V, kr_Z;
  double *kr_w = nullptr, *kr_z = nullptr;
  double **kr_Vtab = nullptr, **kr_Ztab = nullptr;
  double *kr_h = nullptr, *kr_c = nullptr, *kr_n2 = nullptr, *kr_work = nullptr;
  int kr_cap = 0;                    // vectors the tables, coefficient slots and partial sums hold
  long long kr_gs_fused = 0, kr_gs_composed = 0;
  long long n_applies = 0, n_mults = 0, last_applies = 0, last_mults = 0;   // apply() / matmult() calls: ever, and of the last solve()
  void krylov_reserve(int vectors, bool flexible);
  double* krylov_vector(std::vector<double*>& basis, double** tab, int i);
  void krylov_release();
  int solve_gmres_right(const double* b, double* x, KspResult* res, bool flexible);
  // Flexible CG.  Ring slot s (fcg_window.h) holds direction fc_P[s] and its product fc_W[s], each allocated when a step
  // first needs it.  fc_Ptab / fc_Wtab: device tables that name every slot twice (a window is contiguous in them);
  // fc_Btab: per slot the pair {w, r} of the step's two dot products; fc_s: [|r|^2, eta, pi, h_0 .. h_slots-1] so that one
  // download brings the scalars a test needs.  All of it is allocated by the first fcg solve (again when -ksp_fcg_mmax
  // changes the number of slots) and freed by fcg_release (with the set-up).
  std::vector<double*> fc_P, fc_W, fc_Ph, fc_Wh;   // fc_Ph / fc_Wh: host copies of the two doubled tables (composed forms)
  double* fc_r = nullptr;
  double **fc_Ptab = nullptr, **fc_Wtab = nullptr, **fc_Btab = nullptr;
  double *fc_s = nullptr, *fc_c = nullptr, *fc_work = nullptr;
  int fc_slots = 0, fc_max_window = 0;
  long long fc_steps_fused = 0, fc_steps_composed = 0, fc_downloads = 0;
  void fcg_reserve(int slots);
  double* fcg_vector(bool product, int slot);
  void fcg_release();
  int solve_fcg(const double* b, double* x, KspResult* res);
  void free_all();
};

}  // namespace geneo
