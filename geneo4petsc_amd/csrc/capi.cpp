// extern "C" entry points of libgeneopc (declared in include/geneo_c.h).
#include <dlfcn.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <stdexcept>
#include <string>
#include <vector>

#include <algorithm>
#include <chrono>
#include <thread>

#include "../../include/geneo_c.h"
#include "amg.h"
#include "block_dev.h"
#include "krylov_dev.h"
#include "cheb_dev.h"
#include "coarse_dev.h"
#include "core.h"
#include "dense.h"

struct _p_GeneoPC {
  geneo::PC* ctx = nullptr;   // pc->data in PETSc (src/geneo.cpp:2645)
  std::string name, err, optstr;
  // PCSetOperators_GenEO copy (the MATIS A of the one-subdomain-per-rank model)
  bool has_ops = false;
  int nbDOF = 0, nbDOFLoc = 0;
  std::vector<int> map, rowptr, col;
  std::vector<double> val;
  const double* b_dev = nullptr;
};

struct _p_GeneoSpmv {
  bk::Csr a;
};

struct _p_GeneoTestAmg {
  geneo::AmgDevice dev;
  bk::Csr fine;               // the level-0 matrix: uploaded by the hook, borrowed by the hierarchy (fine_dev)
};
static void test_amg_free(_p_GeneoTestAmg* h) {
  if (!h) return;
  h->dev.free_all();          // before the matrix its level 0 borrows
  bk::csr_free(h->fine);
  delete h;
}

static std::string g_global_err;

#define GUARD_BEGIN try {
#define GUARD_END(pc)                                \
  }                                                  \
  catch (std::exception & e) {                       \
    if (pc) (pc)->err = e.what();                    \
    else g_global_err = e.what();                    \
    return 1;                                        \
  }

static int pcfail(PC pc, const std::string& m) {
  if (pc) pc->err = m;
  return 1;
}
static int propagate(PC pc, int rc) {
  if (rc && pc && pc->ctx) pc->err = pc->ctx->last_error;
  return rc;
}

extern "C" {

PetscErrorCode PCCreate_GenEO(PC* pc) {
  if (!pc) return 1;
  *pc = new _p_GeneoPC();
  return createGenEOPC(*pc);
}

PetscErrorCode PCGenEOCreateContext(PC pc) { return createGenEOPC(pc); }
PetscErrorCode createGenEOPC(PC pc) {
  if (!pc) return 1;  // "GenEO preconditioner is invalid"
  delete pc->ctx;
  pc->ctx = new geneo::PC();
  pc->name = pc->ctx->opt.name();
  return 0;
}

PetscErrorCode PCDestroy_GenEO(PC* pc) {
  if (!pc || !*pc) return 0;
  GUARD_BEGIN
  delete (*pc)->ctx;
  delete *pc;
  *pc = nullptr;
  bk::alloc_cache_release();      // blocks parked by the caching allocator go back to the device
  GUARD_END((PC) nullptr)
  return 0;
}

static const char* kFlagOptions[] = {"-geneo_cst", "-geneo_no_syl", "-geneo_offload"};
static bool is_flag(const std::string& k) {
  for (const char* f : kFlagOptions)
    if (k == f) return true;
  return false;
}

PetscErrorCode PCGenEOSetOption(PC pc, const char* key, const char* value) {
  if (!pc || !pc->ctx) return 1;
  const std::string k = key ? key : "", v = value ? value : "";
  std::string e = geneo::parse_option(pc->ctx->opt, k, v);
  if (!e.empty()) return pcfail(pc, e);
  e = geneo::validate_options(pc->ctx->opt);
  if (!e.empty()) return pcfail(pc, e);
  pc->name = pc->ctx->opt.name();
  return 0;
}

PetscErrorCode PCSetFromOptions_GenEO(PC pc, int argc, const char* const* argv) {
  if (!pc || !pc->ctx) return 1;
  for (int i = 0; i < argc; ++i) {
    const std::string k = argv[i] ? argv[i] : "";
    if (k.empty() || k[0] != '-') continue;
    if (is_flag(k)) {
      geneo::parse_option(pc->ctx->opt, k, "");
      continue;
    }
    const bool known = k.rfind("-geneo_", 0) == 0 || k.rfind("-els2_", 0) == 0 || k.rfind("-dls1_", 0) == 0 ||
                       k.rfind("-ksp_", 0) == 0 || k.rfind("-amg_", 0) == 0;
    if (!known) continue;
    if (i + 1 >= argc) return pcfail(pc, "invalid option " + k);
    const std::string v = argv[i + 1];
    std::string e = geneo::parse_option(pc->ctx->opt, k, v);
    if (!e.empty()) {
      if (e.rfind("unknown option", 0) == 0) continue;  // forwarded prefix this build does not use
      return pcfail(pc, e);
    }
    ++i;
  }
  std::string e = geneo::validate_options(pc->ctx->opt);
  if (!e.empty()) return pcfail(pc, e);
  pc->name = pc->ctx->opt.name();
  return 0;
}

const char* PCGenEOGetName(PC pc) { return pc ? pc->name.c_str() : ""; }
const char* PCGenEOGetOptionsString(PC pc) {
  if (!pc || !pc->ctx) return "";
  const geneo::Options& o = pc->ctx->opt;
  char buf[1408];
  snprintf(buf, sizeof(buf),
           "lvl1ASM=%d;lvl1RAS=%d;lvl1SRAS=%d;lvl1ORAS=%d;lvl2=%d;hybrid=%d;effHybrid=%d;optim=%.17g;tau=%.17g;"
           "gamma=%.17g;cst=%d;cut=%d;noSyl=%d;offload=%d;eps_tol=%.17g;dls1_rtol=%.17g;dls1_pc=%s;els2_pc=%s;"
           "ksp_type=%s;ksp_rtol=%.17g;ksp_atol=%.17g;ksp_max_it=%d;ksp_restart=%d;"
           "dls1_ksp_type=%s;dls1_cheb_esteig_its=%d;dls1_cheb_safety=%.17g,%.17g;block_width=%d",
           (int)o.lvl1ASM, (int)o.lvl1RAS, (int)o.lvl1SRAS, (int)o.lvl1ORAS, o.lvl2, (int)o.hybrid, (int)o.effHybrid,
           o.optim, o.tau, o.gamma, (int)o.cst, o.cut, (int)o.noSyl, (int)o.offload, o.eps_tol, o.dls1_rtol,
           o.dls1_pc.c_str(), o.els2_pc.c_str(), o.ksp_type.c_str(), o.ksp_rtol, o.ksp_atol, o.ksp_max_it,
           o.ksp_restart, o.dls1_ksp.c_str(), o.dls1_cheb_esteig_its, o.dls1_cheb_safety_lo, o.dls1_cheb_safety_hi,
           o.block_width);
  pc->optstr = buf;
  if (!o.ksp_matsolve_type.empty()) pc->optstr += ";ksp_matsolve_type=" + o.ksp_matsolve_type;   // only when set
  if (!o.ksp_pc_side.empty()) pc->optstr += ";ksp_pc_side=" + o.ksp_pc_side;                     // likewise
  if (o.ksp_fcg_mmax_set) pc->optstr += ";ksp_fcg_mmax=" + std::to_string(o.ksp_fcg_mmax);
  if (!o.ksp_fcg_truncation.empty()) pc->optstr += ";ksp_fcg_truncation_type=" + o.ksp_fcg_truncation;
  if (!o.ksp_norm_type.empty()) pc->optstr += ";ksp_norm_type=" + o.ksp_norm_type;
  return pc->optstr.c_str();
}
const char* PCGenEOGetError(PC pc) { return pc ? pc->err.c_str() : g_global_err.c_str(); }

const char* usageGenEO_c(void) {
  return "\nusage: GenEO (Domain Decomposition Method) on MI355X\n\n"
         "  -geneo_lvl L1,L2 preconditioner with 2 levels L1 and L2\n"
         "                   L1 = ASM | RAS | SRAS | ORAS | SORAS\n"
         "                   L2 = 0 | 1 | H1 | E1 | 2 | H2 | E2\n"
         "  -geneo_optim A   robin = dirichlet + optim * neumann (ORAS, SORAS; defaults to 0.)\n"
         "  -geneo_tau T     tau threshold (defaults to 0.1)\n"
         "  -geneo_gamma G   gamma threshold (defaults to 10.)\n"
         "  -geneo_cst       do not allow local variations of tau and gamma (GenEO-2)\n"
         "  -geneo_cut C     maximum number of local eigen vectors used to build Z\n"
         "                   (without it every eigenvalue below tau is kept: the LOBPCG block grows up to 64 columns)\n"
         "  -geneo_no_syl    ask for -els2_eps_nev eigenvalues instead (no inertia estimate exists on the GPU path)\n"
         "  -geneo_offload   accepted for compatibility (E is replicated on every GPU)\n"
         "  -geneo_chk F     perform additional checks (F = log | bin | mat; files are text)\n"
         "                     - check partition of unity\n"
         "                     - check matrices are SPD (check.SPD.A.log, check<id>.SPD.<pb>.B.log)\n"
         "                     - check R from Z=QR (check<id>.setup.Z.R, check.setup.ZE2G.R)\n"
         "  -geneo_coarse_device auto|never|always   where the coarse operator E is factored and solved (defaults to auto)\n"
         "                   never:  host Cholesky; sweeps in one workgroup up to dimE 1024, on the host above\n"
         "                   auto:   as never up to dimE 1024; above: blocked factorisation and sweeps on the GPU\n"
         "                   always: the blocked GPU kernels at any dimE (host sequence when E is not positive definite)\n"
         "  -geneo_coarse_block B   block size of the blocked kernels, a multiple of 16 in 16 .. 256 (defaults to 128)\n"
         "  -geneo_block_width W   0 | 16 | 32 (defaults to 0): slab width of the block entry points PCMatApply_GenEO,\n"
         "                   MatMatMult_GenEO and KSPMatSolve_GenEO (several right-hand sides per pass over the matrices); needs\n"
         "                   -dls1_ksp_type chebyshev; read by the set-up, a later change waits for the next set-up; 0 allocates\n"
         "                   and builds nothing\n"
         "  -geneo_nicolaides_zero X   the Nicolaides rule takes min(lambda) >= X eps as 'no zero eigenvalue found'\n"
         "                   (1 = the reference's literal test; defaults to 100)\n"
         "  -geneo_eig_group_rows R / -geneo_eig_mem_gb G   memory-bounded set-up: eigensolve the rank's subdomains in\n"
         "                   consecutive groups of at most R local rows / G GiB of basis blocks (default: 35 % of the card)\n"
         "  -geneo_eig_coarse_start R   subdomains of R rows or more (all of a batch): the local eigensolve starts from the Ritz\n"
         "                   vectors of the multigrid level-1 pencil (itself started from level 2, ...) instead of a random\n"
         "                   block (default 750000; 0 = never)\n"
         "  -els2_eps_tol / -els2_eps_nev / -els2_eps_max_it / -els2_eps_block / -els2_pc_type amg|cheb\n"
         "  -els2_cheb_degree / -els2_cheb_ratio\n"
         "  -dls1_ksp_rtol / -dls1_ksp_max_it / -dls1_pc_type amg|jacobi   local solves (batched PCG)\n"
         "  -dls1_ksp_type cg|chebyshev   the local Krylov method (defaults to cg): batched V-cycle-PCG to -dls1_ksp_rtol, or a\n"
         "                   fixed-degree Chebyshev iteration on the same V-cycle (needs -dls1_pc_type amg): no reductions, no\n"
         "                   host polling, a fixed linear operator at any -dls1_ksp_rtol; the degree per subdomain is the\n"
         "                   smallest k with 1 / T_k(sigma) <= -dls1_ksp_rtol, at most -dls1_ksp_max_it\n"
         "  -dls1_cheb_esteig_its N   Lanczos steps of its eigenvalue-bound estimate (defaults to 16)\n"
         "  -dls1_cheb_safety LO,HI   factors on the smallest and largest Ritz value (defaults to 0.9,1.1; only HI matters for\n"
         "                   positive definiteness, LO for accuracy alone)\n"
         "  -dls1_amg_precision single|double   storage of the matrices its V-cycle reads (arithmetic and vectors: double)\n"
         "  -dls1_amg_strength T / -els2_amg_strength T   aggregation from level 1 on ties |a_ij| >= T 0.5^l sqrt(a_ii a_jj) only\n"
         "  -amg_coarse_size / -amg_smooth_degree / -amg_smooth_ratio / -amg_max_levels\n"
         "  -dls1_amg_smooth_ratio R / -els2_amg_smooth_ratio R   the smoothing interval [rho / R, 1.1 rho] per hierarchy\n"
         "  -ksp_type cg|gmres|fgmres|fcg -ksp_rtol -ksp_atol -ksp_max_it -ksp_gmres_restart\n"
         "  -ksp_type fcg    flexible CG (left-preconditioned, short recurrences, the norms of cg) for the symmetric modes with a\n"
         "                   preconditioner that changes between applications (-dls1_ksp_type cg at a loose -dls1_ksp_rtol);\n"
         "                   not with -ksp_pc_side right or KSPMatSolve_GenEO\n"
         "  -ksp_fcg_mmax M  (defaults to 30, M >= 1) directions a new direction is made conjugate to, at most\n"
         "  -ksp_fcg_truncation_type notay|standard   (defaults to notay) the window grows from 1 to M and starts again, or is\n"
         "                   always the M most recent directions\n"
         "  -ksp_norm_type preconditioned|unpreconditioned   (defaults to preconditioned) unpreconditioned, with -ksp_type fcg\n"
         "                   only: the convergence test and the reported norms are those of the true residual b - A x\n"
         "  -ksp_pc_side left|right   (defaults to left) right with -ksp_type gmres: right-preconditioned GMRES, whose convergence\n"
         "                   test and reported norms are those of the true residual b - A x; -ksp_type fgmres (flexible GMRES,\n"
         "                   for a preconditioner that changes between applications: -dls1_ksp_type cg at a loose -dls1_ksp_rtol)\n"
         "                   is always right; not with -ksp_type cg, -geneo_lvl ...,E1 | E2 or KSPMatSolve_GenEO\n"
         "  -ksp_matsolve_type cg|gmres   the Krylov method of KSPMatSolve_GenEO alone (unset: -ksp_type, which must then be cg);\n"
         "                   gmres: restarted GMRES on every column in lock step, for the non-symmetric modes (RAS, ORAS, hybrid)\n\n";
}

PetscErrorCode PCSetOperators_GenEO(PC pc, const GeneoMatIS* A) {
  if (!pc || !A) return 1;
  if (!A->map || !A->local.rowptr || A->local.n != A->nbDOFLoc)
    return pcfail(pc, "GenEO preconditioner needs the A matrix to be of MATIS type");
  pc->has_ops = true;
  pc->nbDOF = A->nbDOF;
  pc->nbDOFLoc = A->nbDOFLoc;
  pc->map.assign(A->map, A->map + A->nbDOFLoc);
  pc->rowptr.assign(A->local.rowptr, A->local.rowptr + A->nbDOFLoc + 1);
  const int nnz = pc->rowptr[A->nbDOFLoc];
  pc->col.assign(A->local.col, A->local.col + nnz);
  pc->val.assign(A->local.val, A->local.val + nnz);
  return 0;
}

PetscErrorCode PCGenEOSetSizes(PC pc, int nbDOF, int nbSubdomainsGlobal) {
  if (!pc || !pc->ctx) return 1;
  pc->ctx->N = nbDOF;
  pc->ctx->nsub_global = nbSubdomainsGlobal;
  return 0;
}

PetscErrorCode PCGenEOAddSubdomain(PC pc, int gid, int n, const int* map, const int* mult, const GeneoCsr* A,
                                   const GeneoCsr* ADir) {
  if (!pc || !pc->ctx) return 1;
  if (!A || A->n != n) return pcfail(pc, "GenEO preconditioner: bad local matrix");
  if (ADir && ADir->n != n) return pcfail(pc, "GenEO preconditioner: bad dirichlet matrix");
  GUARD_BEGIN
  return propagate(pc, pc->ctx->add_subdomain(gid, n, map, mult, A->rowptr, A->col, A->val,
                                              ADir ? ADir->rowptr : nullptr, ADir ? ADir->col : nullptr,
                                              ADir ? ADir->val : nullptr));
  GUARD_END(pc)
}

PetscErrorCode PCGenEOSetupViews(PC pc, const GeneoCsr* pcADirLoc, GeneoIS mults, const GeneoIS* inters) {
  return PCGenEOSetup(pc, pcADirLoc, mults, inters);
}
PetscErrorCode PCGenEOSetup(PC pc, const GeneoCsr* pcADirLoc, GeneoIS mults, const GeneoIS* inters) {
  if (!pc || !pc->ctx) return 1;
  if (!pc->has_ops) return pcfail(pc, "GenEO preconditioner: PCSetOperators_GenEO must be called first");
  if (mults.n != pc->nbDOFLoc) return pcfail(pc, "Mismatch in dof mult size and local size");
  geneo::PC* c = pc->ctx;
  if (c->N == 0) c->N = pc->nbDOF;
  if (c->nsub_global == 0) c->nsub_global = c->size;
  GeneoCsr a{pc->nbDOFLoc, pc->rowptr.data(), pc->col.data(), pc->val.data()};
  if (PetscErrorCode rc = PCGenEOAddSubdomain(pc, c->rank, pc->nbDOFLoc, pc->map.data(), mults.idx, &a, pcADirLoc))
    return rc;
  if (inters) {  // only the emptiness of each list is used, and only by GenEO-2 (src/geneo.cpp:1139-1148)
    std::vector<int> flags(c->nsub_global);
    for (int q = 0; q < c->nsub_global; ++q) flags[q] = inters[q].n > 0;
    return PCGenEOSetIntersect(pc, c->rank, c->nsub_global, flags.data());
  }
  return 0;
}

PetscErrorCode PCGenEOSetIntersect(PC pc, int gid, int nb, const int* nonempty) {
  if (!pc || !pc->ctx) return 1;
  GUARD_BEGIN
  return propagate(pc, pc->ctx->set_intersect(gid, nb, nonempty));
  GUARD_END(pc)
}

PetscErrorCode initGenEOPC_c(PC pc, unsigned int nbDOF, unsigned int nbDOFLoc, const int* map, const GeneoCsr* A,
                             const GeneoCsr* ADir, const double* b_dev, double* x0_dev, const unsigned int* mult) {
  (void)x0_dev;  // fetched with PCGenEOGetX0 after setup
  if (!pc || !pc->ctx) return 1;
  if (!mult) return pcfail(pc, "GenEO preconditioner without DOF multiplicity");
  geneo::PC* c = pc->ctx;
  c->N = (int)nbDOF;
  if (c->nsub_global == 0) c->nsub_global = c->size;
  std::vector<int> m(mult, mult + nbDOFLoc);
  pc->b_dev = b_dev;
  return PCGenEOAddSubdomain(pc, c->rank, (int)nbDOFLoc, map, m.data(), A, ADir);
}

PetscErrorCode PCGenEOSetComm(PC pc, int rank, int size, int n_owned, const int* owned_gid, int n_halo,
                              const int* halo_gid, const int* recv_counts, const int* send_counts,
                              const int* send_idx, GeneoExchangeFn exchange, GeneoAllreduceFn allreduce, void* user,
                              double* send_dev, double* recv_dev, double* red_dev, int red_capacity) {
  if (!pc || !pc->ctx) return 1;
  geneo::PC* c = pc->ctx;
  if (size < 1 || rank < 0 || rank >= size) return pcfail(pc, "GenEO: bad communicator");
  if (size > 1 && (red_capacity < 1 || !red_dev || !exchange || !allreduce))
    return pcfail(pc, "GenEO: communicator needs both callbacks and a reduction buffer of at least one double");
  c->rank = rank;
  c->size = size;
  c->owned.assign(owned_gid, owned_gid + n_owned);
  c->halo_gid.assign(halo_gid, halo_gid + n_halo);
  if (size > 1) {
    c->recv_counts.assign(recv_counts, recv_counts + size);
    c->send_counts.assign(send_counts, send_counts + size);
    int ns = 0;
    for (int q = 0; q < size; ++q) ns += send_counts[q];
    c->send_idx.assign(send_idx, send_idx + ns);
  }
  c->cb_exchange = exchange;
  c->cb_allreduce = allreduce;
  c->cb_user = user;
  c->comm_send = send_dev;
  c->comm_recv = recv_dev;
  c->comm_red = red_dev;
  c->comm_red_cap = red_capacity;
  return 0;
}

PetscErrorCode PCGenEOSetCommWidth(PC pc, int max_width) {
  if (!pc || !pc->ctx) return 1;
  if (max_width < 1) return pcfail(pc, "GenEO: bad halo buffer width");
  pc->ctx->comm_width = max_width;
  return 0;
}

PetscErrorCode PCGenEOSetRHS(PC pc, const double* b_dev) {
  if (!pc) return 1;
  pc->b_dev = b_dev;
  return 0;
}

PetscErrorCode PCSetUp_GenEO(PC pc) {
  if (!pc || !pc->ctx) return 1;
  GUARD_BEGIN
  geneo::PC* c = pc->ctx;
  if (c->nsub_global == 0) c->nsub_global = (int)c->subs.size();
  return propagate(pc, c->setup(pc->b_dev));
  GUARD_END(pc)
}
PetscErrorCode PCApply_GenEO(PC pc, const double* x, double* y) {
  if (!pc || !pc->ctx) return 1;
  GUARD_BEGIN
  return propagate(pc, pc->ctx->apply(x, y));
  GUARD_END(pc)
}
PetscErrorCode PCGenEOApplyQ(PC pc, const double* x, double* y) {
  if (!pc || !pc->ctx) return 1;
  GUARD_BEGIN
  return propagate(pc, pc->ctx->apply_q(x, y));
  GUARD_END(pc)
}
PetscErrorCode MatMult_GenEO(PC pc, const double* x, double* y) {
  if (!pc || !pc->ctx) return 1;
  GUARD_BEGIN
  return propagate(pc, pc->ctx->matmult(x, y));
  GUARD_END(pc)
}
PetscErrorCode PCGenEOGetX0(PC pc, double* x0_dev) {
  if (!pc || !pc->ctx || !pc->ctx->x0_dev()) return 1;
  GUARD_BEGIN
  bk::d2d(x0_dev, pc->ctx->x0_dev(), sizeof(double) * pc->ctx->n_owned());
  GUARD_END(pc)
  return 0;
}
PetscErrorCode KSPSolve_GenEO(PC pc, const double* b, double* x, int* its, double* rnorm, int* reason) {
  if (!pc || !pc->ctx) return 1;
  GUARD_BEGIN
  geneo::KspResult r;
  int rc = pc->ctx->solve(b, x, &r);
  if (its) *its = r.its;
  if (rnorm) *rnorm = r.rnorm;
  if (reason) *reason = r.reason;
  return propagate(pc, rc);
  GUARD_END(pc)
}
PetscErrorCode PCMatApply_GenEO(PC pc, const double* X, int ldx, double* Y, int ldy, int m) {
  if (!pc || !pc->ctx) return 1;
  GUARD_BEGIN
  return propagate(pc, pc->ctx->apply_mat(X, ldx, Y, ldy, m));
  GUARD_END(pc)
}
PetscErrorCode MatMatMult_GenEO(PC pc, const double* X, int ldx, double* Y, int ldy, int m) {
  if (!pc || !pc->ctx) return 1;
  GUARD_BEGIN
  return propagate(pc, pc->ctx->matmult_mat(X, ldx, Y, ldy, m));
  GUARD_END(pc)
}
PetscErrorCode KSPMatSolve_GenEO(PC pc, const double* B, int ldb, double* X, int ldx, int m, int* its, double* rnorm,
                                 int* reason) {
  if (!pc || !pc->ctx) return 1;
  GUARD_BEGIN
  return propagate(pc, pc->ctx->solve_mat(B, ldb, X, ldx, m, its, rnorm, reason));
  GUARD_END(pc)
}
int PCGenEOGetBlockInfo(PC pc, int* width, long long* slabs, long long* columns, long long* padded, long long* graph_launches) {
  if (!pc || !pc->ctx) return -1;
  pc->ctx->block_info(width, slabs, columns, padded, graph_launches);
  return 0;
}
int PCGenEOGetBlockKrylovInfo(PC pc, int* basis_slabs, double* basis_bytes, long long* gs_fused, long long* gs_composed) {
  if (!pc || !pc->ctx) return -1;
  pc->ctx->block_krylov_info(basis_slabs, basis_bytes, gs_fused, gs_composed);
  return 0;
}
int PCGenEOGetKrylovInfo(PC pc, int* basis_vectors, double* basis_bytes, long long* gs_fused, long long* gs_composed,
                         long long* pc_applies, long long* mat_mults) {
  if (!pc || !pc->ctx) return -1;
  pc->ctx->krylov_info(basis_vectors, basis_bytes, gs_fused, gs_composed, pc_applies, mat_mults);
  return 0;
}
int PCGenEOGetFcgInfo(PC pc, int* directions, double* bytes, long long* steps_fused, long long* steps_composed, int* max_window,
                      long long* downloads) {
  if (!pc || !pc->ctx) return -1;
  pc->ctx->fcg_info(directions, bytes, steps_fused, steps_composed, max_window, downloads);
  return 0;
}
int PCGenEOGetCoarseBlockCounters(PC pc, long long* blocked, long long* by_column, long long* host_blocks) {
  if (!pc || !pc->ctx) return -1;
  pc->ctx->coarse_block_counters(blocked, by_column, host_blocks);
  return 0;
}
int PCGenEOGetResidualHistory(PC pc, double* hist, int cap) {
  if (!pc || !pc->ctx) return 0;
  const auto& h = pc->ctx->residual_history;
  for (int i = 0; i < (int)h.size() && i < cap; ++i) hist[i] = h[i];
  return (int)h.size();
}

PetscErrorCode PCGenEOGetInfo(PC pc, GeneoInfo* o) {
  if (!pc || !pc->ctx || !o) return 1;
  const geneo::Info& i = pc->ctx->info;
  o->estimDimELoc = i.estimDimELoc; o->realDimELoc = i.realDimELoc; o->nicolaidesLoc = i.nicolaidesLoc;
  o->dimE = i.dimE; o->eig_iterations = i.eig_iterations; o->eig_spmm = i.eig_spmm;
  o->dls1_iterations = i.dls1_iterations; o->dls1_solves = i.dls1_solves; o->spmv_calls = i.spmv_calls;
  o->lvl1SetupMinvTimeLoc = i.lvl1SetupMinvTimeLoc; o->lvl2SetupEigTimeLoc = i.lvl2SetupEigTimeLoc;
  o->lvl2SetupZTimeLoc = i.lvl2SetupZTimeLoc; o->lvl2SetupETimeLoc = i.lvl2SetupETimeLoc;
  o->lvl1ApplyTimeLoc = i.lvl1ApplyTimeLoc; o->lvl1ApplyScatterTimeLoc = i.lvl1ApplyScatterTimeLoc;
  o->lvl1ApplyMinvTimeLoc = i.lvl1ApplyMinvTimeLoc; o->lvl1ApplyGatherTimeLoc = i.lvl1ApplyGatherTimeLoc;
  o->lvl1ApplyPrjFSTimeLoc = i.lvl1ApplyPrjFSTimeLoc; o->lvl2ApplyTimeLoc = i.lvl2ApplyTimeLoc;
  o->lvl2ApplyZtTimeLoc = i.lvl2ApplyZtTimeLoc; o->lvl2ApplyEinvTimeLoc = i.lvl2ApplyEinvTimeLoc;
  o->lvl2ApplyZTimeLoc = i.lvl2ApplyZTimeLoc; o->setupTime = i.setupTime; o->solveTime = i.solveTime;
  o->amg_levels = i.amg_levels; o->amg_operator_complexity = i.amg_operator_complexity; o->amgSetupTime = i.amgSetupTime;
  o->nullPivotsLoc = i.nullPivotsLoc;
  o->eigGroups = i.eig_groups;
  o->eigCoarseIterations = i.eig_coarse_iterations;
  return 0;
}
static int copy_out(const std::vector<double>& v, double* out, int cap) {
  for (int i = 0; i < (int)v.size() && i < cap; ++i) out[i] = v[i];
  return (int)v.size();
}
int PCGenEOGetEigenvalues(PC pc, int s, double* vals, int cap) {
  if (!pc || !pc->ctx || s < 0 || s >= (int)pc->ctx->eigvals.size()) return -1;
  return copy_out(pc->ctx->eigvals[s], vals, cap);
}
int PCGenEOGetCandidates(PC pc, int s, double* vals, int cap) {
  if (!pc || !pc->ctx || s < 0 || s >= (int)pc->ctx->candidates.size()) return -1;
  return copy_out(pc->ctx->candidates[s], vals, cap);
}
int PCGenEOGetE(PC pc, double* e, int cap) {
  if (!pc || !pc->ctx) return -1;
  copy_out(pc->ctx->E, e, cap);
  return pc->ctx->info.dimE;
}
int PCGenEOGetLocalParams(PC pc, double* tau, double* gamma, int cap) {
  if (!pc || !pc->ctx) return -1;
  const auto& t = pc->ctx->tauLoc;
  const auto& g = pc->ctx->gammaLoc;
  for (int i = 0; i < (int)t.size() && i < cap; ++i) {
    if (tau) tau[i] = t[i];
    if (gamma) gamma[i] = i < (int)g.size() ? g[i] : -1.0;
  }
  return (int)t.size();
}
int PCGenEOGetLocalDims(PC pc, int* k, int cap) {
  if (!pc || !pc->ctx) return -1;
  const auto& v = pc->ctx->ksub_global;
  for (int i = 0; i < (int)v.size() && i < cap; ++i) k[i] = v[i];
  return (int)v.size();
}

int PCGenEOGetLocalSolverInfo(PC pc, double* lo, double* hi, int* its, double* achieved, int cap) {
  if (!pc || !pc->ctx) return -1;
  const geneo::PC& c = *pc->ctx;
  const int n = (int)c.cheb_its.size();
  for (int i = 0; i < n && i < cap; ++i) {
    if (lo) lo[i] = c.cheb_lo[i];
    if (hi) hi[i] = c.cheb_hi[i];
    if (its) its[i] = c.cheb_its[i];
    if (achieved) achieved[i] = i < (int)c.cheb_achieved.size() ? c.cheb_achieved[i] : 0.0;
  }
  return n;
}

int PCGenEOGetLocalSolverTable(PC pc, double* coef, int cap) {
  if (!pc || !pc->ctx) return -1;
  const int K = pc->ctx->cheb_steps_per_solve();
  if (coef && K > 0) {
    try {
      const std::vector<double> t = pc->ctx->cheb_table();
      std::copy_n(t.begin(), std::min<size_t>(t.size(), (size_t)std::max(0, cap)), coef);
    } catch (std::exception& e) {
      pcfail(pc, e.what());
      return -1;
    }
  }
  return K;
}

int PCGenEOGetLocalSolverCounters(PC pc, long long* solves, long long* graph_launches, long long* fused_residuals) {
  if (!pc || !pc->ctx) return -1;
  long long v[3];
  pc->ctx->cheb_counters(&v[0], &v[1], &v[2]);
  if (solves) *solves = v[0];
  if (graph_launches) *graph_launches = v[1];
  if (fused_residuals) *fused_residuals = v[2];
  return pc->ctx->cheb_steps_per_solve();
}

PetscErrorCode PCGenEOGetCoarseInfo(PC pc, int* dimE, int* factor_on_device, int* solve_kind, int* block) {
  if (!pc || !pc->ctx) return 1;
  pc->ctx->coarse_info(dimE, factor_on_device, solve_kind, block);
  return 0;
}

// ---- getInput plugin ABI (driver:75-96) -----------------------------------------------------------
// Loads a plugin built for the reference driver (tst/laplacian, tst/heat, tst/graph or a user's own) and
// flattens what it returns.  The C++ signature is the plugin contract itself (driver:81-85).
typedef int (*geneo_get_input_fn)(std::string const& args, unsigned int& nbElem, unsigned int& nbNode,
                                  std::vector<unsigned int>& elemPtr, std::vector<unsigned int>& elemIdx,
                                  std::vector<std::vector<double>>& elemSubMat);
PetscErrorCode GeneoGetLibInput(const char* inpLibA, const char* inpLibArg, GeneoInput* out) {
  if (!inpLibA || !out) return 1;
  memset(out, 0, sizeof(*out));
  void* lib = dlopen(inpLibA, RTLD_LAZY | RTLD_LOCAL);
  if (!lib) {
    g_global_err = std::string("Error: open library KO - ") + dlerror();
    return 1;
  }
  geneo_get_input_fn fn = (geneo_get_input_fn)dlsym(lib, "getInput");
  if (!fn) {
    g_global_err = std::string("Error: get input function from library KO - ") + dlerror();
    dlclose(lib);
    return 1;
  }
  std::string args = inpLibArg ? inpLibArg : "";
  for (auto& c : args)
    if (c == '#') c = ' ';
  unsigned int ne = 0, nn = 0;
  std::vector<unsigned int> ptr, idx;
  std::vector<std::vector<double>> sub;
  int rc = 1;
  try {
    rc = fn(args, ne, nn, ptr, idx, sub);
  } catch (std::exception& e) {
    g_global_err = e.what();
  }
  if (rc != 0 || ptr.size() != (size_t)ne + 1 || sub.size() != ne) {
    if (g_global_err.empty() || rc != 0) g_global_err = "Error: get input data from library KO";
    dlclose(lib);
    return 1;
  }
  size_t tot = 0;
  for (auto& m : sub) tot += m.size();
  out->nbElem = ne;
  out->nbNode = nn;
  out->nIdx = idx.size();
  out->nMat = tot;
  out->elemPtr = (unsigned int*)malloc(sizeof(unsigned int) * (ptr.size() + 1));
  out->elemIdx = (unsigned int*)malloc(sizeof(unsigned int) * (idx.size() + 1));
  out->elemMat = (double*)malloc(sizeof(double) * (tot + 1));
  memcpy(out->elemPtr, ptr.data(), sizeof(unsigned int) * ptr.size());
  memcpy(out->elemIdx, idx.data(), sizeof(unsigned int) * idx.size());
  size_t pos = 0;
  for (auto& m : sub) {
    memcpy(out->elemMat + pos, m.data(), sizeof(double) * m.size());
    pos += m.size();
  }
  dlclose(lib);
  return 0;
}
void GeneoFreeInput(GeneoInput* in) {
  if (!in) return;
  free(in->elemPtr);
  free(in->elemIdx);
  free(in->elemMat);
  memset(in, 0, sizeof(*in));
}

// ---- device helpers ------------------------------------------------------------------------
const char* GeneoBackendName(void) { return bk::name(); }
PetscErrorCode GeneoSetStream(void* s) {
  bk::set_stream(s);
  return 0;
}
int GeneoDeviceCount(void) { return bk::device_count(); }
int GeneoSetDevice(int local_rank) { return bk::set_device(local_rank); }
int GeneoCurrentDevice(void) { return bk::current_device(); }
int GeneoThreadDeviceCheck(void) { return bk::thread_device_check(); }
void GeneoAllocCacheRelease(void) { bk::alloc_cache_release(); }
void* GeneoDeviceAlloc(size_t bytes) {
  try {
    return bk::alloc(bytes);
  } catch (std::exception& e) {
    g_global_err = e.what();
    return nullptr;
  }
}
void GeneoDeviceFree(void* p) { bk::dfree(p); }
PetscErrorCode GeneoH2D(void* d, const void* s, size_t b) {
  GUARD_BEGIN
  bk::h2d(d, s, b);
  GUARD_END((PC) nullptr)
  return 0;
}
PetscErrorCode GeneoD2H(void* d, const void* s, size_t b) {
  GUARD_BEGIN
  bk::d2h(d, s, b);
  GUARD_END((PC) nullptr)
  return 0;
}
PetscErrorCode GeneoDeviceSync(void) {
  GUARD_BEGIN
  bk::sync();
  GUARD_END((PC) nullptr)
  return 0;
}
int GeneoSelfTestMFMA(void) {
  try {
    return bk::selftest_mfma_f64();
  } catch (std::exception& e) {
    g_global_err = e.what();
    return -1;
  }
}
PetscErrorCode GeneoTestAxpby(double* y_dev, const double* x_dev, double a, double b, int n) {
  GUARD_BEGIN
  bk::axpby(y_dev, a, x_dev, b, n);
  GUARD_END((PC) nullptr)
  return 0;
}
PetscErrorCode GeneoSetSpmvKind(int kind) {
  bk::set_spmv_kind(kind);
  return 0;
}
const char* GeneoSpmvKernelName(void) { return bk::spmv_kernel_name(); }
PetscErrorCode GeneoSetMFMA(int enable) {
  bk::set_mfma(enable != 0);
  return 0;
}
PetscErrorCode GeneoSetKernelVariant(const char* name, int value) {
  if (name && std::string(name) == "cheb_fused") {     // a choice of core.cpp, not of the backend: bk::cheb_dir / bk::cheb_residual or their composed forms
    geneo::set_cheb_fused(value);
    return 0;
  }
  if (name && std::string(name) == "block_fused") {    // likewise: the kernels of block_dev.h or their composed forms
    geneo::set_block_fused(value);
    return 0;
  }
  if (name && std::string(name) == "krylov_fused") {   // likewise: the kernels of krylov_dev.h or their composed forms
    geneo::set_krylov_fused(value);
    return 0;
  }
  return bk::set_variant(name, value) ? 0 : 1;
}

// ---- stand-alone kernels --------------------------------------------------------------------
PetscErrorCode GeneoSpmvCreate(const GeneoCsr* a, GeneoSpmv* h) {
  if (!a || !h) return 1;
  GUARD_BEGIN
  *h = new _p_GeneoSpmv();
  (*h)->a = bk::csr_upload(a->n, a->rowptr, a->col, a->val);
  GUARD_END((PC) nullptr)
  return 0;
}
PetscErrorCode GeneoSpmvApply(GeneoSpmv h, const double* x, double* y) {
  if (!h) return 1;
  GUARD_BEGIN
  bk::spmv(h->a, x, y);
  GUARD_END((PC) nullptr)
  return 0;
}
PetscErrorCode GeneoSpmvTime(GeneoSpmv h, const double* x, double* y, int reps, double* ms_avg) {
  if (!h || reps < 1) return 1;
  GUARD_BEGIN
  void* e0 = bk::event_create();
  void* e1 = bk::event_create();
  bk::spmv(h->a, x, y);  // warm
  bk::event_record(e0);
  for (int i = 0; i < reps; ++i) bk::spmv(h->a, x, y);
  bk::event_record(e1);
  const float ms = bk::event_elapsed_ms(e0, e1);
  bk::event_destroy(e0);
  bk::event_destroy(e1);
  if (ms_avg) *ms_avg = (double)ms / reps;
  GUARD_END((PC) nullptr)
  return 0;
}
PetscErrorCode GeneoSpmvProfileStart(int every, double min_bytes) {
  bk::spmv_profile_start(every, min_bytes);
  return 0;
}
PetscErrorCode GeneoSpmvProfileStop(double* ms_sum, double* bytes_sum, long long* nsampled, long long* nlaunch) {
  GUARD_BEGIN
  bk::spmv_profile_stop(ms_sum, bytes_sum, nsampled, nlaunch);
  GUARD_END((PC) nullptr)
  return 0;
}
PetscErrorCode GeneoDeviceMemInfo(double* live, double* live_peak, double* footprint_peak, double* cached, double* dev_free,
                                  double* dev_total, int reset_peaks) {
  GUARD_BEGIN
  bk::mem_info(live, live_peak, footprint_peak, cached, dev_free, dev_total, reset_peaks != 0);
  GUARD_END((PC) nullptr)
  return 0;
}
PetscErrorCode GeneoKernelProfileStart(int every, double spmv_min_bytes) {
  GUARD_BEGIN
  bk::kernel_profile_start(every, spmv_min_bytes);
  GUARD_END((PC) nullptr)
  return 0;
}
PetscErrorCode GeneoKernelProfileStop(void) {
  GUARD_BEGIN
  bk::kernel_profile_stop();
  GUARD_END((PC) nullptr)
  return 0;
}
PetscErrorCode GeneoKernelProfileGet(int kernel_class, double* ms_sum, double* bytes_sum, double* flops_sum,
                                     long long* nsampled, long long* nlaunch) {
  GUARD_BEGIN
  bk::kernel_profile_get(kernel_class, ms_sum, bytes_sum, flops_sum, nsampled, nlaunch);
  GUARD_END((PC) nullptr)
  return 0;
}
PetscErrorCode GeneoSpmvDestroy(GeneoSpmv* h) {
  if (!h || !*h) return 0;
  bk::csr_free((*h)->a);
  delete *h;
  *h = nullptr;
  return 0;
}
PetscErrorCode GeneoSpmmApply(GeneoSpmv h, const double* X, double* Y, int m, const double* pre, const double* post) {
  if (!h) return 1;
  GUARD_BEGIN
  bk::spmm_strided(h->a, X, m, Y, m, m, pre, post);
  GUARD_END((PC) nullptr)
  return 0;
}

// strided blocks + HIP-event timing of `reps` back-to-back launches (reps <= 0: one untimed launch)
PetscErrorCode GeneoSpmmTime(GeneoSpmv h, const double* X, int ldx, double* Y, int ldy, int m, const double* pre,
                             const double* post, int reps, double* ms_avg) {
  if (!h) return 1;
  GUARD_BEGIN
  bk::spmm_strided(h->a, X, ldx, Y, ldy, m, pre, post);
  if (reps > 0) {
    void* e0 = bk::event_create();
    void* e1 = bk::event_create();
    bk::event_record(e0);
    for (int i = 0; i < reps; ++i) bk::spmm_strided(h->a, X, ldx, Y, ldy, m, pre, post);
    bk::event_record(e1);
    const float ms = bk::event_elapsed_ms(e0, e1);
    bk::event_destroy(e0);
    bk::event_destroy(e1);
    if (ms_avg) *ms_avg = (double)ms / reps;
  }
  GUARD_END((PC) nullptr)
  return 0;
}

PetscErrorCode GeneoSpmmFused(GeneoSpmv h, int epi, const double* X, double* Y, int m, const double* B, double* Z,
                              const double* dinv, double w) {
  if (!h) return 1;
  GUARD_BEGIN
  bk::spmm_fused(h->a, epi, X, m, Y, m, m, B, m, Z, m, dinv, w);
  GUARD_END((PC) nullptr)
  return 0;
}

// the same single-vector launches reading the single-precision companion of the matrix (built on first use); epi 0: Y = A X
// Y1 = B X and Y2 = A X in one pass over X, B laid out on A's sliced pattern (bk::sell_values_on + bk::spmm_dual: LOBPCG's
// A W / B W pass).  Returns 2 when pattern(B) is not contained in pattern(A) or A is not on the sliced path.
PetscErrorCode GeneoSpmmDualTest(GeneoSpmv a, GeneoSpmv b, const double* X, int ldx, double* Y1, double* Y2, int ldy, int m) {
  if (!a || !b) return 1;
  GUARD_BEGIN
  if (!bk::spmm_dual_available(a->a, m)) return 2;
  double* v = bk::sell_values_on(a->a, b->a);
  if (!v) return 2;
  bk::spmm_dual(a->a, v, a->a.sl_val, X, ldx, Y1, Y2, ldy, m);
  bk::sync();
  bk::dfree(v);
  GUARD_END((PC) nullptr)
  return 0;
}
// R = mask .* (A X - B X diag(lam)) per subdomain (suboff: nsub + 1 first rows; lam, mask: nsub x m host arrays), both
// products in one pass over X and neither written (bk::spmm_dual_residual: the residual block of LOBPCG's lean iteration)
PetscErrorCode GeneoSpmmDualResidualTest(GeneoSpmv a, GeneoSpmv b, const double* X, int ldx, double* R, int ldr, int m,
                                         int nsub, const int* suboff, const double* lam, const double* mask) {
  if (!a || !b) return 1;
  GUARD_BEGIN
  if (!bk::spmm_dual_available(a->a, m)) return 2;
  double* v = bk::sell_values_on(a->a, b->a);
  if (!v) return 2;
  bk::Chunks c = bk::chunks_upload(nsub, suboff);
  double* dl = (double*)bk::alloc(sizeof(double) * (size_t)nsub * m);
  double* dm = (double*)bk::alloc(sizeof(double) * (size_t)nsub * m);
  bk::h2d(dl, lam, sizeof(double) * (size_t)nsub * m);
  bk::h2d(dm, mask, sizeof(double) * (size_t)nsub * m);
  bk::spmm_dual_residual(a->a, a->a.sl_val, v, X, ldx, R, ldr, m, c, dl, dm);
  bk::sync();
  bk::dfree(v); bk::dfree(dl); bk::dfree(dm);
  bk::chunks_free(c);
  GUARD_END((PC) nullptr)
  return 0;
}
PetscErrorCode GeneoSpmvFusedSingle(GeneoSpmv h, int epi, const double* X, double* Y, const double* B, double* Z,
                                    const double* dinv, double w) {
  if (!h) return 1;
  GUARD_BEGIN
  if (!bk::csr_has_lp(h->a) && !bk::csr_make_lp(h->a))
    throw std::runtime_error("no single-precision companion for this matrix (ragged or long rows: not on the sliced path)");
  if (epi == 0) bk::spmv_lp(h->a, X, Y);
  else bk::spmv_fused_lp(h->a, epi, X, Y, B, Z, dinv, w);
  GUARD_END((PC) nullptr)
  return 0;
}

PetscErrorCode GeneoSpmvOffsetInfo(GeneoSpmv h, int* slices, int* coded) {
  if (!h) return 1;
  if (slices) *slices = h->a.nslice;
  if (coded) *coded = h->a.off_coded;
  return 0;
}

// test hook for the device sparse products: op 0: C = A B, op 1: C = A^T (B ignored).  Returns nnz(C) (-1: a row
// exceeded the kernels' capacity, -2: error); fills the outputs when cap >= nnz (rowptr_out has C's rows + 1 entries).
long long GeneoTestSparseProduct(int op, const GeneoCsr* A, const GeneoCsr* B, int ncols, int* rowptr_out, int* col_out,
                                 double* val_out, long long cap) {
  try {
    bk::Csr a = bk::csr_upload_raw(A->n, A->rowptr, A->col, A->val);     // CSR arrays only: the products read nothing else
    bk::Csr b;
    if (op == 0) b = bk::csr_upload_raw(B->n, B->rowptr, B->col, B->val);
    bool ok = true;
    bk::Csr c = (op == 0) ? bk::spgemm(a, b, ncols, &ok) : bk::transpose(a, ncols, &ok);
    long long nnz = ok ? (long long)c.nnz : -1;
    if (ok && cap >= nnz && rowptr_out) bk::csr_download(c, rowptr_out, col_out, val_out);
    bk::csr_free(a);
    if (op == 0) bk::csr_free(b);
    if (ok) bk::csr_free(c);
    return nnz;
  } catch (std::exception& e) {
    g_global_err = e.what();
    return -2;
  }
}

// what the calling thread's last sparse product decided (bk::sparse_product_report); any pointer may be NULL
int GeneoTestSparseProductReport(int* group, int* deferred, int* scan_depth) {
  const bk::SparseProductReport r = bk::sparse_product_report();
  if (group) *group = r.group;
  if (deferred) *deferred = r.deferred;
  if (scan_depth) *scan_depth = r.scan_depth;
  return 0;
}

// threshold (chunks per subdomain) above which the per-subdomain reductions take their cooperative forms; returns the
// previous value.  Set it BEFORE creating the PC whose solves it should govern (captured HIP graphs keep their launches).
int GeneoSetParReduceMin(int chunks) {
  const int old = bk::get_par_reduce_min();
  bk::set_par_reduce_min(chunks);
  return old;
}
// test hook of the fused LOBPCG update (m = 32): host arrays in, host arrays out
PetscErrorCode GeneoTestLobpcgUpdate(int nsub, const int* suboff, const double* S, const double* AS, const double* BS,
                                     const double* C, const double* keep, const double* lam, const double* mask,
                                     double* T, double* AT, double* BT, double* R) {
  GUARD_BEGIN
  if (!bk::lobpcg_update32_available()) throw std::runtime_error("fused LOBPCG update unavailable (MFMA off)");
  const int n = suboff[nsub];
  bk::Chunks c = bk::chunks_upload(nsub, suboff);
  auto up = [](const double* h, size_t k) {
    double* d = (double*)bk::alloc(sizeof(double) * std::max<size_t>(1, k));
    if (h) bk::h2d(d, h, sizeof(double) * k);
    return d;
  };
  const size_t nb = (size_t)n * 96;
  if (!AS) {   // the basis-only form of the lean iteration: T = [X' P'] from S (AS, BS, lam, mask, AT, BT, R unused)
    double *dS = up(S, nb), *dC = up(C, (size_t)nsub * 96 * 64), *dk = up(keep, (size_t)nsub * 32), *dT = up(nullptr, nb);
    bk::lobpcg_update32_basis(c, dS, dC, dk, dT);
    bk::d2h(T, dT, sizeof(double) * nb);
    for (double* d : {dS, dC, dk, dT}) bk::dfree(d);
    bk::chunks_free(c);
    return 0;
  }
  double *dS = up(S, nb), *dAS = up(AS, nb), *dBS = up(BS, nb), *dC = up(C, (size_t)nsub * 96 * 64);
  double *dk = up(keep, (size_t)nsub * 32), *dl = up(lam, (size_t)nsub * 32), *dm = up(mask, (size_t)nsub * 32);
  double *dT = up(nullptr, nb), *dAT = up(nullptr, nb), *dBT = up(nullptr, nb), *dR = up(nullptr, (size_t)n * 32);
  bk::lobpcg_update32(c, dS, dAS, dBS, dC, dk, dl, dm, dT, dAT, dBT, dR);
  bk::d2h(T, dT, sizeof(double) * nb);
  bk::d2h(AT, dAT, sizeof(double) * nb);
  bk::d2h(BT, dBT, sizeof(double) * nb);
  bk::d2h(R, dR, sizeof(double) * (size_t)n * 32);
  for (double* d : {dS, dAS, dBS, dC, dk, dl, dm, dT, dAT, dBT, dR}) bk::dfree(d);
  bk::chunks_free(c);
  GUARD_END((PC) nullptr)
  return 0;
}

PetscErrorCode GeneoBlockKernel(int kind, int nsub, const int* suboff, const double* S, int p, const double* TC, int q,
                                double* out, int reps, double* ms_avg) {
  GUARD_BEGIN
  const int n = suboff[nsub];
  bk::Chunks c = bk::chunks_upload(nsub, suboff);
  double* dS = (double*)bk::alloc(sizeof(double) * (size_t)n * p);
  bk::h2d(dS, S, sizeof(double) * (size_t)n * p);
  void* e0 = bk::event_create();
  void* e1 = bk::event_create();
  if (kind == 0 || kind == 2) {
    // kind 2: the left operand as TWO strided views (columns [0, p/2) and [p/2, p) of S: what LOBPCG passes as A W, B W)
    double* dT = (double*)bk::alloc(sizeof(double) * (size_t)n * q);
    double* dG = (double*)bk::alloc(sizeof(double) * (size_t)nsub * p * q);
    bk::h2d(dT, TC, sizeof(double) * (size_t)n * q);
    auto run = [&]() {
      if (kind == 0) bk::gram(c, dS, p, p, dT, q, q, dG);
      else bk::gram2(c, dS, p, p / 2, dS + p / 2, p, p - p / 2, dT, q, q, dG);
    };
    run();
    if (reps > 0) {
      bk::event_record(e0);
      for (int i = 0; i < reps; ++i) run();
      bk::event_record(e1);
      if (ms_avg) *ms_avg = bk::event_elapsed_ms(e0, e1) / reps;
    }
    bk::d2h(out, dG, sizeof(double) * (size_t)nsub * p * q);
    bk::dfree(dT);
    bk::dfree(dG);
  } else {
    double* dC = (double*)bk::alloc(sizeof(double) * (size_t)nsub * p * q);
    double* dY = (double*)bk::alloc(sizeof(double) * (size_t)n * q);
    bk::h2d(dC, TC, sizeof(double) * (size_t)nsub * p * q);
    bk::block_mul(c, dS, p, p, dC, q, dY, q, false);
    if (reps > 0) {
      bk::event_record(e0);
      for (int i = 0; i < reps; ++i) bk::block_mul(c, dS, p, p, dC, q, dY, q, false);
      bk::event_record(e1);
      if (ms_avg) *ms_avg = bk::event_elapsed_ms(e0, e1) / reps;
    }
    bk::d2h(out, dY, sizeof(double) * (size_t)n * q);
    bk::dfree(dC);
    bk::dfree(dY);
  }
  bk::dfree(dS);
  bk::chunks_free(c);
  bk::event_destroy(e0);
  bk::event_destroy(e1);
  GUARD_END((PC) nullptr)
  return 0;
}

// ---- test hooks of the backend primitives (tests/primitive_cases.py) ---------------------------------------------------
// No arithmetic here: arguments are unpacked, bk:: is called, results stay where the primitive wrote them.  Every pointer
// in parg is a device pointer of the caller (GeneoDeviceAlloc) except parg[0] of the chunked primitives: the HOST array
// suboff (iarg[0] = nsub), from which the bk::Chunks is built around the call.
// Returns the primitive's own result (void: 0, bool: 0 / 1, recip_positive: its count), -1 on an exception (message:
// PCGenEOGetError(NULL)), -2 for an unknown name.
int GeneoTestPrimitive(const char* name, const int* I, const double* D, void* const* P) {
  const std::string k(name ? name : "");
  auto d = [&](int i) { return (double*)P[i]; };
  auto ip = [&](int i) { return (int*)P[i]; };
  auto lp = [&](int i) { return (int64_t*)P[i]; };
  bk::Chunks c;
  bool have_chunks = false;
  int rc = 0;
  try {
    // ---- plain vectors and blocks
    if (k == "gather") bk::gather(d(0), d(1), ip(2), I[0]);
    else if (k == "gather_mul") bk::gather_mul(d(0), d(1), ip(2), d(3), I[0]);
    else if (k == "segsum") bk::segsum(d(0), d(1), ip(2), ip(3), I[0], I[1] != 0);
    else if (k == "gather_rows") bk::gather_rows(d(0), d(1), ip(2), I[0], I[1]);
    else if (k == "segsum_rows") bk::segsum_rows(d(0), d(1), ip(2), ip(3), I[0], I[1], I[2] != 0);
    else if (k == "set") bk::set(d(0), D[0], I[0]);
    else if (k == "zero") bk::zero(P[0], (size_t)I[0]);
    else if (k == "copy") bk::copy(d(0), d(1), I[0]);
    else if (k == "axpy") bk::axpy(d(0), D[0], d(1), I[0]);
    else if (k == "axpby") bk::axpby(d(0), D[0], d(1), D[1], I[0]);
    else if (k == "xmy") bk::xmy(d(0), d(1), d(2), I[0]);
    else if (k == "axpy_dev") bk::axpy_dev(d(0), d(1), D[0], d(2), I[0]);
    else if (k == "dot") bk::dot(d(0), d(1), I[0], d(2));
    else if (k == "block_axpby") bk::block_axpby(d(0), I[0], D[0], d(1), I[1], D[1], I[2], I[3]);
    else if (k == "block_rowscale") bk::block_rowscale(d(0), I[0], d(1), I[1], d(2), D[0], D[1], I[2], I[3]);
    else if (k == "jacobi_step") bk::jacobi_step(d(0), I[0], d(1), I[1], d(2), d(3), D[0], I[2], I[3], I[4] != 0);
    else if (k == "cheb_update") bk::cheb_update(d(0), d(1), d(2), d(3), I[0], d(4), D[0], D[1], I[1], I[2]);
    else if (k == "chol_solve") rc = bk::chol_solve(d(0), d(1), I[0], d(2)) ? 1 : 0;
    else if (k == "recip_positive") rc = bk::recip_positive(d(0), I[0]);
    else {
      // ---- chunked primitives
      c = bk::chunks_upload(I[0], (const int*)P[0]);
      have_chunks = true;
      if (k == "seg_dot") bk::seg_dot(c, d(1), d(2), d(3), I[1], I[2]);
      else if (k == "dense_sym_apply") bk::dense_sym_apply(c, d(1), lp(2), d(3), I[1], d(4), I[2], I[3]);
      else if (k == "gram") bk::gram(c, d(1), I[1], I[2], d(2), I[3], I[4], d(3));
      else if (k == "block_mul") bk::block_mul(c, d(1), I[1], I[2], d(2), I[3], d(3), I[4], I[5] != 0);
      else if (k == "block_residual") bk::block_residual(c, d(1), I[1], d(2), I[2], d(3), I[3], d(4), I[4], d(5));
      else if (k == "block_colnorm") bk::block_colnorm(c, d(1), I[1], I[2], d(2));
      else if (k == "block_residual_norms")
        bk::block_residual_norms(c, d(1), I[1], d(2), I[2], d(3), I[3], d(4), I[4], d(5), d(6));
      else if (k == "block_colscale") bk::block_colscale(c, d(1), I[1], I[2], d(2));
      else if (k == "cheb_dir")      // (GeneoSetKernelVariant("cheb_fused", 0): the composed form of core.cpp)
        rc = (geneo::cheb_fused() ? bk::cheb_dir(c, d(1), I[1], d(2), d(3), d(4), d(5), d(6))
                                  : geneo::cheb_dir_composed_once(c, d(1), I[1], d(2), d(3), d(4), d(5), d(6), 1)) ? 1 : 0;
      else if (k == "block_init")
        bk::block_init(c, d(1), I[1], I[2], ip(2), ((uint64_t)(uint32_t)I[4] << 32) | (uint64_t)(uint32_t)I[3]);
      else if (k == "block_extract") bk::block_extract(c, d(1), I[1], I[2], d(2), ip(3), ip(4), lp(5), d(6));
      else if (k == "z_rowmajor") bk::z_rowmajor(c, d(1), lp(2), ip(3), d(4), I[1]);
      else if (k == "zt_apply") bk::zt_apply(c, d(1), lp(2), ip(3), ip(4), I[1], d(5), d(6), I[2]);
      else if (k == "z_apply") bk::z_apply(c, d(1), lp(2), ip(3), ip(4), d(5), d(6), I[1] != 0);
      else rc = -2;
    }
    bk::sync();
  } catch (std::exception& e) {
    g_global_err = e.what();
    rc = -1;
  }
  if (have_chunks) bk::chunks_free(c);
  return rc;
}

// ---- test hook of the block primitives (block_dev.h; argument tables: tests/block_rhs_util.py, and
// tests/block_gmres_util.py for block_gs_dots, block_gs_update, block_scale_cols and block_gs_group) ----------------------
// As GeneoTestPrimitive: unpack, call, leave the results where the primitive wrote them.  "block_fused" 0 runs the composed
// forms of core.cpp instead.  Returns 0 / 1 (the primitive's bool), -1 on an exception, -2 for an unknown name.
int GeneoTestBlockPrimitive(const char* name, const int* I, const double* D, void* const* P) {
  (void)D;
  const std::string k(name ? name : "");
  auto d = [&](int i) { return (double*)P[i]; };
  const bool fused = geneo::block_fused() != 0;
  bk::Chunks c;
  bool have_chunks = false;
  int rc = 0;
  try {
    if (k == "cheb_dir_block") {
      c = bk::chunks_upload(I[0], (const int*)P[0]);
      have_chunks = true;
      rc = (fused ? bk::cheb_dir_block(c, d(1), I[1], d(2), d(3), d(4), d(5), d(6), I[2])
                  : geneo::cheb_dir_composed_once(c, d(1), I[1], d(2), d(3), d(4), d(5), d(6), I[2])) ? 1 : 0;
    } else if (k == "block_import") {
      rc = (fused ? bk::block_import(d(0), I[0], I[1], I[2], d(1), I[3])
                  : geneo::block_import_composed(d(0), I[0], I[1], I[2], d(1), I[3])) ? 1 : 0;
    } else if (k == "block_export") {
      rc = (fused ? bk::block_export(d(0), I[3], I[1], I[2], d(1), I[0])
                  : geneo::block_export_composed(d(0), I[3], I[1], I[2], d(1), I[0])) ? 1 : 0;
    } else if (k == "block_coldot") {
      if (fused) {
        double* work = (double*)bk::alloc(sizeof(double) * (size_t)bk::BLOCK_COLDOT_WG * I[1]);
        try {
          rc = bk::block_coldot(d(0), d(1), I[0], I[1], d(2), work) ? 1 : 0;
          bk::sync();
        } catch (...) {
          bk::dfree(work);
          throw;
        }
        bk::dfree(work);
      } else {
        rc = geneo::block_coldot_composed_once(d(0), d(1), I[0], I[1], d(2)) ? 1 : 0;
      }
    } else if (k == "block_axpy_cols") {
      rc = (fused ? bk::block_axpy_cols(d(0), d(1), d(2), I[0], I[1])
                  : geneo::block_axpy_cols_composed_once(d(0), d(1), d(2), I[0], I[1])) ? 1 : 0;
    } else if (k == "block_xpby_cols") {
      rc = (fused ? bk::block_xpby_cols(d(0), d(1), d(2), I[0], I[1])
                  : geneo::block_xpby_cols_composed_once(d(0), d(1), d(2), I[0], I[1])) ? 1 : 0;
    } else if (k == "block_gs_group") {                // the group size of bk::block_gs_dots, as the return value
      rc = bk::BLOCK_GS_GROUP;
    } else if (k == "block_gs_dots") {                 // I(nb, n, w)  P(V table, W, H, work)
      rc = (fused ? bk::block_gs_dots((const double* const*)P[0], I[0], d(1), I[1], I[2], d(2), d(3))
                  : geneo::block_gs_dots_composed_once((const double* const*)P[0], I[0], d(1), I[1], I[2], d(2), d(3))) ? 1 : 0;
    } else if (k == "block_gs_update") {               // I(nb, n, w)  P(Y, V table, C, norm2 | NULL, work | NULL)
      rc = (fused ? bk::block_gs_update(d(0), (const double* const*)P[1], I[0], d(2), I[1], I[2], d(3), d(4))
                  : geneo::block_gs_update_composed_once(d(0), (const double* const*)P[1], I[0], d(2), I[1], I[2], d(3), d(4))) ? 1 : 0;
    } else if (k == "block_scale_cols") {              // I(n, w)  P(Out, X, c)
      rc = (fused ? bk::block_scale_cols(d(0), d(1), d(2), I[0], I[1])
                  : geneo::block_scale_cols_composed_once(d(0), d(1), d(2), I[0], I[1])) ? 1 : 0;
    } else if (k == "chol_solve_block") {
      rc = (fused ? bk::chol_solve_block(d(0), d(1), I[0], d(2), I[1])
                  : geneo::chol_solve_block_composed_once(d(0), d(1), I[0], d(2), I[1])) ? 1 : 0;
    } else {
      rc = -2;
    }
    bk::sync();
  } catch (std::exception& e) {
    g_global_err = e.what();
    rc = -1;
  }
  if (have_chunks) bk::chunks_free(c);
  return rc;
}

// ---- test hook of the Gram-Schmidt primitives of the right-preconditioned GMRES (krylov_dev.h; argument table:
// tests/krylov_right_util.py) -------------------------------------------------------------------------------------------
// As GeneoTestBlockPrimitive.  "krylov_fused" 0 runs the composed forms of core.cpp instead.
int GeneoTestKrylovPrimitive(const char* name, const int* I, const double* D, void* const* P) {
  (void)D;
  const std::string k(name ? name : "");
  auto d = [&](int i) { return (double*)P[i]; };
  const bool fused = geneo::krylov_fused() != 0;
  int rc = 0;
  try {
    if (k == "vec_gs_group") {                         // the group size of bk::vec_gs_dots, as the return value
      rc = bk::VEC_GS_GROUP;
    } else if (k == "vec_dot_nwg") {                   // I(n): the workgroups (partial sums per vector) of a pass over n rows
      rc = bk::vec_dot_nwg(I[0]);
    } else if (k == "vec_gs_dots") {                   // I(nb, n)  P(V table, W, H, work)
      rc = (fused ? bk::vec_gs_dots((const double* const*)P[0], I[0], d(1), I[1], d(2), d(3))
                  : geneo::vec_gs_dots_composed_once((const double* const*)P[0], I[0], d(1), I[1], d(2))) ? 1 : 0;
    } else if (k == "vec_gs_update") {                 // I(nb, n)  P(Y, V table, C, norm2 | NULL, work | NULL)
      rc = (fused ? bk::vec_gs_update(d(0), (const double* const*)P[1], I[0], d(2), I[1], d(3), d(4))
                  : geneo::vec_gs_update_composed_once(d(0), (const double* const*)P[1], I[0], d(2), I[1], d(3))) ? 1 : 0;
    } else if (k == "vec_fcg_step") {                  // I(n)  P(x, r, p, w, S, norm2 | NULL, work | NULL)
      rc = (fused ? bk::vec_fcg_step(d(0), d(1), d(2), d(3), d(4), I[0], d(5), d(6))
                  : geneo::vec_fcg_step_composed(d(0), d(1), d(2), d(3), d(4), I[0], d(5))) ? 1 : 0;
    } else {
      rc = -2;
    }
    bk::sync();
  } catch (std::exception& e) {
    g_global_err = e.what();
    rc = -1;
  }
  return rc;
}

// ---- test hooks of the blocked coarse kernels (coarse_dev.h; tests/test_gpu_coarse_device.py) ---------------------------
// Host arrays in and out.  Every device buffer is allocated with CANARY_PAD doubles (ints for the status word) in front and
// behind, filled with a canary pattern, and read back whole: a broken canary or a changed input is an error (-1).
// nb == 0 runs what the PC does without these kernels instead -- dense::cholesky_blocked and the transposition; the download,
// dense::cholesky_solve_lu and the upload -- so that the two can be timed and compared by one caller.
namespace {
static constexpr size_t CANARY_PAD = 64;
static const double kCanary = -6.02214076e+231;
static const int kCanaryInt = 0x5ca1ab1e;
static double g_coarse_factor_ms = -1.0, g_coarse_solve_ms = -1.0;

struct PaddedBuf {          // device buffer of n doubles between two canary pads
  double* d = nullptr;
  size_t n = 0;
  std::vector<double> h;
  PaddedBuf(size_t n_, const double* src) : n(n_), h(n_ + 2 * CANARY_PAD, kCanary) {
    if (src) std::copy(src, src + n, h.begin() + CANARY_PAD);
    d = (double*)bk::alloc(sizeof(double) * h.size());
    bk::h2d(d, h.data(), sizeof(double) * h.size());
  }
  ~PaddedBuf() { bk::dfree(d); }
  double* ptr() { return d + CANARY_PAD; }
  // reads the buffer back; throws when a pad was written (or, with `same`, when the payload differs from it)
  const double* fetch(const char* what, const double* same = nullptr) {
    bk::d2h(h.data(), d, sizeof(double) * h.size());
    for (size_t i = 0; i < CANARY_PAD; ++i)
      if (std::memcmp(&h[i], &kCanary, 8) || std::memcmp(&h[CANARY_PAD + n + i], &kCanary, 8))
        throw std::runtime_error(std::string("coarse test hook: write outside ") + what);
    if (same && n && std::memcmp(h.data() + CANARY_PAD, same, sizeof(double) * n))
      throw std::runtime_error(std::string("coarse test hook: input changed: ") + what);
    return h.data() + CANARY_PAD;
  }
};
double wall_ms(std::chrono::steady_clock::time_point a) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - a).count();
}
}  // namespace

int GeneoTestCoarseFactor(int n, int nb, const double* E, double* L, double* LT, int* status) {
  try {
    if (n < 0 || !E || !L || !LT || !status) throw std::runtime_error("GeneoTestCoarseFactor: bad arguments");
    const size_t nn = (size_t)n * n;
    if (nb == 0) {     // the host factorisation of PC::build_E
      std::vector<double> a(E, E + nn);
      const auto t0 = std::chrono::steady_clock::now();
      const bool ok = dense::cholesky_blocked(a, n, (int)std::min(16u, std::max(1u, std::thread::hardware_concurrency())));
      std::fill(LT, LT + nn, 0.0);
      for (int i = 0; i < n; ++i)
        for (int j = 0; j <= i; ++j) LT[(size_t)j * n + i] = a[(size_t)i * n + j];
      g_coarse_factor_ms = wall_ms(t0);
      for (int i = 0; i < n; ++i)       // the host routine leaves E above the diagonal, where nothing of the PC reads
        std::fill(a.begin() + (size_t)i * n + i + 1, a.begin() + (size_t)(i + 1) * n, 0.0);
      std::copy(a.begin(), a.end(), L);
      *status = ok ? 0 : n;      // the host routine keeps no pivot index
      return 0;
    }
    PaddedBuf dE(nn, E), dL(nn, nullptr), dLT(nn, nullptr);
    std::vector<int> hs(1 + 2 * CANARY_PAD, kCanaryInt);
    int* dst = (int*)bk::alloc(sizeof(int) * hs.size());
    bk::h2d(dst, hs.data(), sizeof(int) * hs.size());
    void* e0 = bk::event_create();
    void* e1 = bk::event_create();
    bk::event_record(e0);
    const bool have = bk::coarse_factor(dE.ptr(), n, nb, dL.ptr(), dLT.ptr(), dst + CANARY_PAD);
    bk::event_record(e1);
    if (have) {
      g_coarse_factor_ms = (double)bk::event_elapsed_ms(e0, e1);
      bk::d2h(hs.data(), dst, sizeof(int) * hs.size());
    }
    bk::event_destroy(e0);
    bk::event_destroy(e1);
    bk::dfree(dst);
    if (!have) return -3;
    for (size_t i = 0; i < CANARY_PAD; ++i)
      if (hs[i] != kCanaryInt || hs[CANARY_PAD + 1 + i] != kCanaryInt)
        throw std::runtime_error("coarse test hook: write outside the status word");
    *status = hs[CANARY_PAD];
    dE.fetch("E", E);
    std::copy_n(dL.fetch("L"), nn, L);
    std::copy_n(dLT.fetch("LT"), nn, LT);
    return 0;
  } catch (std::exception& e) {
    g_global_err = e.what();
    return -1;
  }
}

int GeneoTestCoarseSolve(int n, int nb, const double* L, const double* LT, double* y, int reps) {
  try {
    if (n < 0 || !L || !LT || !y || reps < 1) throw std::runtime_error("GeneoTestCoarseSolve: bad arguments");
    const size_t nn = (size_t)n * n;
    PaddedBuf dy0(n, y), dy(n, nullptr);
    if (nb == 0) {     // the host round trip of PC::coarse_solve_local
      const std::vector<double> l(L, L + nn), u(LT, LT + nn);
      std::vector<double> hy(std::max(1, n));
      const auto t0 = std::chrono::steady_clock::now();
      for (int r = 0; r < reps; ++r) {
        bk::d2h(hy.data(), dy0.ptr(), sizeof(double) * n);
        dense::cholesky_solve_lu(l, u, n, hy.data());
        bk::h2d(dy.ptr(), hy.data(), sizeof(double) * n);
      }
      bk::sync();
      g_coarse_solve_ms = wall_ms(t0) / reps;
      std::copy_n(dy.fetch("y"), n, y);
      return 0;
    }
    PaddedBuf dL(nn, L), dLT(nn, LT);
    void* e0 = bk::event_create();
    void* e1 = bk::event_create();
    bool have = true;
    bk::event_record(e0);
    for (int r = 0; r < reps && have; ++r) {   // every repetition solves the caller's y again
      bk::d2d(dy.ptr(), dy0.ptr(), sizeof(double) * n);
      have = bk::coarse_solve(dL.ptr(), dLT.ptr(), n, nb, dy.ptr());
    }
    bk::event_record(e1);
    if (have) g_coarse_solve_ms = (double)bk::event_elapsed_ms(e0, e1) / reps;
    bk::event_destroy(e0);
    bk::event_destroy(e1);
    if (!have) return -3;
    dL.fetch("L", L);
    dLT.fetch("LT", LT);
    dy0.fetch("y (input copy)", y);
    std::copy_n(dy.fetch("y"), n, y);
    return 0;
  } catch (std::exception& e) {
    g_global_err = e.what();
    return -1;
  }
}

// The blocked sweeps on the n x w row-major block Y (bk::coarse_solve_block); the device time of one repetition goes where
// GeneoTestCoarseSolve puts its own.
int GeneoTestCoarseSolveBlock(int n, int nb, int w, const double* L, const double* LT, double* Y, int reps) {
  try {
    if (n < 0 || w < 1 || !L || !LT || !Y || reps < 1) throw std::runtime_error("GeneoTestCoarseSolveBlock: bad arguments");
    const size_t nn = (size_t)n * n, nw = (size_t)n * w;
    PaddedBuf dy0(nw, Y), dy(nw, nullptr), dL(nn, L), dLT(nn, LT);
    void* e0 = bk::event_create();
    void* e1 = bk::event_create();
    bool have = true;
    std::string err;
    bk::event_record(e0);
    try {
      for (int r = 0; r < reps && have; ++r) {   // every repetition solves the caller's Y again
        bk::d2d(dy.ptr(), dy0.ptr(), sizeof(double) * nw);
        have = bk::coarse_solve_block(dL.ptr(), dLT.ptr(), n, nb, dy.ptr(), w);
      }
    } catch (std::exception& e) {
      err = e.what();
    }
    bk::event_record(e1);
    if (have && err.empty()) g_coarse_solve_ms = (double)bk::event_elapsed_ms(e0, e1) / reps;
    bk::event_destroy(e0);
    bk::event_destroy(e1);
    if (!err.empty()) throw std::runtime_error(err);
    if (!have) return -3;
    dL.fetch("L", L);
    dLT.fetch("LT", LT);
    dy0.fetch("Y (input copy)", Y);
    std::copy_n(dy.fetch("Y"), nw, Y);
    return 0;
  } catch (std::exception& e) {
    g_global_err = e.what();
    return -1;
  }
}

int GeneoTestCoarseElapsed(double* factor_ms, double* solve_ms) {
  if (factor_ms) *factor_ms = g_coarse_factor_ms;
  if (solve_ms) *solve_ms = g_coarse_solve_ms;
  return 0;
}

// The batched CG of the local solves on the matrix of `h` (rows 0 .. suboff[nsub]): cg_start, then `iters` times
// [spmv, seg_pap, cg_update, cg_direction] with alternating parity, ONE bk::Chunks alive across the sequence (it carries
// the chunk partials).  caller_precond != 0: the caller-preconditioned form -- cg_start / cg_update with dinv == nullptr,
// z = dinv .* r by bk::xmy, seg_partial(r, z, 1), cg_set_rz and p = z after the start (the order of PC::local_solve).
// x, r, z, p, b, dinv: device vectors; sc_out: host, nsub x 8.
PetscErrorCode GeneoTestCgSteps(GeneoSpmv h, int nsub, const int* suboff, int iters, double tol2, int caller_precond,
                                const double* b, const double* dinv, double* x, double* r, double* z, double* p,
                                double* sc_out) {
  if (!h) return 1;
  GUARD_BEGIN
  const int n = suboff[nsub], n0 = suboff[0];
  bk::Chunks c = bk::chunks_upload(nsub, suboff);
  double* sc = (double*)bk::alloc(sizeof(double) * 8 * (size_t)std::max(1, nsub));
  double* q = (double*)bk::alloc(sizeof(double) * (size_t)std::max(1, n));
  const double* dv = caller_precond ? nullptr : dinv;
  bk::cg_start(c, sc, x, r, z, p, b, dv);
  if (caller_precond) {
    bk::xmy(z + n0, r + n0, dinv + n0, n - n0);
    bk::seg_partial(c, r, z, 1);
    bk::cg_set_rz(c, sc);
    bk::copy(p + n0, z + n0, n - n0);
  }
  int parity = 0;
  for (int it = 0; it < iters; ++it) {
    bk::spmv(h->a, p, q);
    bk::seg_pap(c, p, q);
    bk::cg_update(c, sc, parity, x, r, z, p, q, dv);
    if (caller_precond) {
      bk::xmy(z + n0, r + n0, dinv + n0, n - n0);
      bk::seg_partial(c, r, z, 1);
    }
    bk::cg_direction(c, sc, parity, p, z, tol2);
    parity ^= 1;
  }
  bk::d2h(sc_out, sc, sizeof(double) * 8 * (size_t)nsub);
  bk::dfree(sc);
  bk::dfree(q);
  bk::chunks_free(c);
  GUARD_END((PC) nullptr)
  return 0;
}

// Set-up operations on CSR matrices (host CSR in, host CSR out; parg: device arrays of the caller).  Returns the number of
// entries of the result and fills the outputs when cap allows (as GeneoTestSparseProduct), -1: a sparse product exceeded
// the kernels' capacity, -2: error, -3: post_matrix returned false.
//   op 0  csr_remap_columns(A, parg[0])
//   op 1  csr_scaled_alias(A, parg[0], parg[1], iarg[0]); iarg[1] = m > 0: then spmm_fused(alias, EPI_PRE) with
//         Y = parg[2] (ld iarg[2]), B = parg[3] (ld iarg[3]), Z = parg[4] (ld iarg[4]; may be null), dinv = parg[5], w = darg[0]
//   op 2  csr_tentative_prolongator(A.n, agg = parg[0]); iarg[1] != 0: spgemm(A, P0, iarg[0] aggregates) and
//         smooth_prolongator(., agg, dinv = parg[1], w = darg[0])
//   op 3  post_matrix(AP = A, P = B, dinv = parg[0], w = darg[0])
//   op 4  csr_diag(A, parg[0])                                    (returns nnz(A), no CSR output)
//   op 5  C = spgemm(A, B, iarg[0]); csr_finish(C); spmv(C, parg[0], parg[1])
long long GeneoTestCsrOp(int op, const GeneoCsr* A, const GeneoCsr* B, const int* iarg, const double* darg,
                         void* const* parg, int* rowptr_out, int* col_out, double* val_out, long long cap) {
  try {
    const bool layouts = (op == 0 || op == 1);   // the SpMV layouts travel with these two
    bk::Csr a = layouts ? bk::csr_upload(A->n, A->rowptr, A->col, A->val) : bk::csr_upload_raw(A->n, A->rowptr, A->col, A->val);
    bk::Csr b, c;
    long long nnz = -2;
    auto out = [&](const bk::Csr& m) {
      nnz = (long long)m.nnz;
      if (cap >= nnz && rowptr_out) bk::csr_download(m, rowptr_out, col_out, val_out);
    };
    if (op == 0) {
      c = bk::csr_remap_columns(a, (const int*)parg[0]);
      out(c);
      bk::csr_free(c);
    } else if (op == 1) {
      c = bk::csr_scaled_alias(a, (const double*)parg[0], (const double*)parg[1], iarg[0] != 0);
      if (iarg[1] > 0)
        bk::spmm_fused(c, bk::EPI_PRE, nullptr, 0, (double*)parg[2], iarg[2], iarg[1], (const double*)parg[3], iarg[3],
                       (double*)parg[4], iarg[4], (const double*)parg[5], darg[0]);
      out(c);
      bk::csr_free(c);
    } else if (op == 2) {
      b = bk::csr_tentative_prolongator(A->n, (const int*)parg[0]);
      if (iarg[1]) {
        bool ok = true;
        c = bk::spgemm(a, b, iarg[0], &ok);
        if (ok) {
          bk::smooth_prolongator(c, (const int*)parg[0], (const double*)parg[1], darg[0]);
          out(c);
          bk::csr_free(c);
        } else nnz = -1;
      } else out(b);
      bk::csr_free(b);
    } else if (op == 3) {
      b = bk::csr_upload_raw(B->n, B->rowptr, B->col, B->val);
      if (bk::post_matrix(a, b, (const double*)parg[0], darg[0])) out(a);
      else nnz = -3;
      bk::csr_free(b);
    } else if (op == 4) {
      bk::csr_diag(a, (double*)parg[0]);
      nnz = (long long)a.nnz;
    } else if (op == 5) {
      b = bk::csr_upload_raw(B->n, B->rowptr, B->col, B->val);
      bool ok = true;
      c = bk::spgemm(a, b, iarg[0], &ok);
      if (ok) {
        bk::csr_finish(c);
        bk::spmv(c, (const double*)parg[0], (double*)parg[1]);
        out(c);
        bk::csr_free(c);
      } else nnz = -1;
      bk::csr_free(b);
    }
    bk::sync();
    bk::csr_free(a);
    return nnz;
  } catch (std::exception& e) {
    g_global_err = e.what();
    return -2;
  }
}

// ---- a stand-alone multigrid hierarchy (test hook): created from a host matrix, read back level by level, and its cycle
// applied to host blocks.  No arithmetic here: upload, AmgDevice, download.
int GeneoTestAmgCreate(const GeneoCsr* A, int nsub, const int* suboff, const int* iparam, const double* dparam,
                       GeneoTestAmg* out) {
  if (!out) return 1;
  *out = nullptr;
  _p_GeneoTestAmg* h = nullptr;
  try {
    if (!A || !suboff || !iparam || !dparam || nsub < 1 || A->n < 1) throw std::runtime_error("GeneoTestAmgCreate: bad arguments");
    if (suboff[0] != 0 || suboff[nsub] != A->n) throw std::runtime_error("GeneoTestAmgCreate: suboff must run from 0 to the matrix size");
    for (int s = 0; s < nsub; ++s)
      if (suboff[s + 1] < suboff[s]) throw std::runtime_error("GeneoTestAmgCreate: suboff must ascend");
    geneo::HostCsr ha;
    ha.n = A->n;
    ha.rowptr.assign(A->rowptr, A->rowptr + A->n + 1);
    ha.col.assign(A->col, A->col + A->rowptr[A->n]);
    ha.val.assign(A->val, A->val + A->rowptr[A->n]);
    geneo::AmgParams prm;
    prm.coarse_size = iparam[0];
    prm.smooth_degree = iparam[1];
    prm.max_levels = iparam[2];
    prm.single = iparam[3] != 0;
    const int max_m = iparam[4];
    prm.smooth_ratio = dparam[0];
    prm.strength = dparam[1];
    const std::vector<int> so(suboff, suboff + nsub + 1);
    h = new _p_GeneoTestAmg();
    h->fine = bk::csr_upload(A->n, A->rowptr, A->col, A->val);
    if (iparam[6] && !bk::csr_make_lp(h->fine)) throw std::runtime_error("GeneoTestAmgCreate: no single-precision companion for the fine matrix");
    bool built = true;
    if (iparam[5] == 0) {
      built = h->dev.build_on_device(ha, so, prm, max_m, &h->fine);
    } else {
      std::vector<geneo::AmgLevelHost> levels;
      std::vector<double> cinv;
      std::vector<int64_t> cbase;
      geneo::amg_setup_host(ha, so, prm, levels, cinv, cbase);
      h->dev.upload(levels, cinv, cbase, prm, max_m, &h->fine);
    }
    bk::sync();
    if (!built) {
      test_amg_free(h);
      return 2;
    }
    *out = h;
    return 0;
  } catch (std::exception& e) {
    g_global_err = e.what();
    try { test_amg_free(h); } catch (...) {}
    return 1;
  }
}

int GeneoTestAmgDestroy(GeneoTestAmg* h) {
  if (!h || !*h) return 0;
  GUARD_BEGIN
  test_amg_free(*h);
  *h = nullptr;
  GUARD_END((PC) nullptr)
  return 0;
}

int GeneoTestAmgInfo(GeneoTestAmg h, int* nlevels, double* operator_complexity, int* lp_matrices) {
  if (!h) return 1;
  if (nlevels) *nlevels = h->dev.nlevels();
  if (operator_complexity) *operator_complexity = h->dev.operator_complexity();
  if (lp_matrices) *lp_matrices = h->dev.lp_matrices();
  return 0;
}

static const bk::Csr* test_amg_matrix(_p_GeneoTestAmg* h, int level, int which) {
  if (level < 0 || level >= h->dev.nlevels()) throw std::runtime_error("GeneoTestAmg: no such level");
  switch (which) {
    case 0: return &h->dev.level_A(level);
    case 1: return &h->dev.level_P(level);
    case 2: return &h->dev.level_R(level);
    case 3: return &h->dev.level_M(level);
    case 4: return &h->dev.level_Acs(level);
  }
  throw std::runtime_error("GeneoTestAmg: no such matrix");
}

int GeneoTestAmgLevel(GeneoTestAmg h, int level, long long* iout, double* rho, int* suboff, double* dinv) {
  if (!h) return 1;
  GUARD_BEGIN
  const bk::Csr& a = *test_amg_matrix(h, level, 0);
  const std::vector<int>& so = h->dev.level_suboff(level);
  const int n = h->dev.level_rows(level);
  if (iout) {
    iout[0] = n;
    iout[1] = (long long)so.size() - 1;
    iout[2] = h->dev.level_fused(level) ? 1 : 0;
    iout[3] = a.vec_lpr;
    iout[4] = a.nlong;
    iout[5] = 0;
    for (int w = 0; w < 5; ++w) {
      const bk::Csr& m = *test_amg_matrix(h, level, w);
      iout[6 + w] = m.n ? (long long)m.nnz : -1;          // -1: the level has no such matrix
      if (m.n && bk::csr_has_lp(m)) iout[5] |= 1LL << w;
    }
  }
  if (rho) *rho = h->dev.level_rho(level);
  if (suboff) std::copy(so.begin(), so.end(), suboff);
  if (dinv) bk::d2h(dinv, h->dev.level_dinv(level), sizeof(double) * (size_t)n);
  GUARD_END((PC) nullptr)
  return 0;
}

long long GeneoTestAmgMatrix(GeneoTestAmg h, int level, int which, int* rows, int* rowptr, int* col, double* val, long long cap) {
  if (!h) return -2;
  try {
    const bk::Csr& m = *test_amg_matrix(h, level, which);
    if (!m.n) return -1;
    if (rows) *rows = m.n;
    if (cap >= (long long)m.nnz && rowptr && col && val) bk::csr_download(m, rowptr, col, val);
    return (long long)m.nnz;
  } catch (std::exception& e) {
    g_global_err = e.what();
    return -2;
  }
}

long long GeneoTestAmgCoarseInverse(GeneoTestAmg h, long long* base, double* inv, long long cap) {
  if (!h || !base) return -2;
  try {
    static_assert(sizeof(long long) == sizeof(int64_t), "bases are downloaded as they lie");
    const int nsub = (int)h->dev.level_suboff(h->dev.nlevels() - 1).size() - 1;
    bk::d2h(base, h->dev.coarsest_inv_base(), sizeof(int64_t) * ((size_t)nsub + 1));
    if (cap >= base[nsub] && inv) bk::d2h(inv, h->dev.coarsest_inv(), sizeof(double) * (size_t)base[nsub]);
    return base[nsub];
  } catch (std::exception& e) {
    g_global_err = e.what();
    return -2;
  }
}

int GeneoTestAmgVcycle(GeneoTestAmg h, int level, double* B, int ldb, double* X, int ldx, int m) {
  if (!h) return 1;
  GUARD_BEGIN
  if (!B || !X || m < 1 || ldb < m || ldx < m) throw std::runtime_error("GeneoTestAmgVcycle: bad arguments");
  if (level < 0 || level >= h->dev.nlevels()) throw std::runtime_error("GeneoTestAmg: no such level");
  const size_t n = (size_t)h->dev.level_rows(level);
  double *b = nullptr, *x = nullptr;
  try {
    b = (double*)bk::alloc(sizeof(double) * n * ldb);
    x = (double*)bk::alloc(sizeof(double) * n * ldx);
    bk::h2d(b, B, sizeof(double) * n * ldb);
    bk::h2d(x, X, sizeof(double) * n * ldx);
    h->dev.vcycle_from(level, b, ldb, x, ldx, m);
    bk::d2h(X, x, sizeof(double) * n * ldx);
    bk::d2h(B, b, sizeof(double) * n * ldb);
  } catch (...) {
    bk::dfree(b);
    bk::dfree(x);
    throw;
  }
  bk::dfree(b);
  bk::dfree(x);
  GUARD_END((PC) nullptr)
  return 0;
}

}  // extern "C"
