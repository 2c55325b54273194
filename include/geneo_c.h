/*
 * geneo_c.h -- C ABI of libgeneopc, the MI355X-native GenEO preconditioner.
 *
 * Drop-in boundary for the PC-shell API of geneo4PETSc:
 *     reference hdr/geneo_c.h:9   PetscErrorCode createGenEOPC(PC);
 *     reference hdr/geneo_c.h:10  PetscErrorCode PCGenEOSetup(PC, Mat, IS, IS*);
 * and for the four callbacks createGenEOPC wires into the PETSc PC (src/geneo.cpp:2717-2720):
 *     ops->setfromoptions = setUpGenEOPCFromOptions   -> PCSetFromOptions_GenEO
 *     ops->setup          = setUpGenEOPC              -> PCSetUp_GenEO
 *     ops->apply          = applyGenEOPC              -> PCApply_GenEO
 *     ops->destroy        = destroyGenEOPC            -> PCDestroy_GenEO
 *
 * PETSc is not available on the GPU box, so the PETSc object types are replaced by plain C
 * views (pointers and sizes, no PETSc and no torch types).  With PETSc present, the adapter in
 * INTEGRATION.md pulls these views out of Mat/IS/Vec and forwards to the same entry points.
 *
 * Conventions
 *   - every function returns PetscErrorCode (int): 0 = success; on failure the message is
 *     available through PCGenEOGetError (the reference aborts through SETERRABORT,
 *     src/geneo.cpp:74; a library must not abort the host process).
 *   - host pointers are read during the call and never retained (the reference borrows
 *     pcA / pcMap / dofIdxMultLoc / intersectLoc, src/geneo.cpp:2221-2230; here they are copied).
 *   - pointers named *_dev are device (HBM) pointers of this process' GPU; vectors are FP64.
 *   - one subdomain per rank is the reference's model; this library also accepts several
 *     subdomains per rank/GPU (PCGenEOAddSubdomain), which is how one MI355X runs a whole
 *     decomposition.
 *   - not re-entrant; one context per PC; collective over the ranks given to PCGenEOSetComm.
 */
#ifndef __GENEOPC_C_ABI_H
#define __GENEOPC_C_ABI_H   /* not the reference guard (__GENEO_C_H): the PETSc-side adapter includes both headers */

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The handle.  Stand-alone it carries PETSc's names (PC, PetscErrorCode) so that host code reads like the reference's.
 * Next to the real PETSc headers (adapters/geneo_petsc_adapter.cpp) define GENEO_HAVE_PETSC before including this file:
 * PETSc's own PC / PetscErrorCode are then left alone and the handle is called GeneoPC. */
#ifdef GENEO_HAVE_PETSC
typedef struct _p_GeneoPC* GeneoPC;
#define GENEO_PC GeneoPC
#else
typedef int PetscErrorCode;
typedef struct _p_GeneoPC* PC;         /* stands for PETSc's PC */
#define GENEO_PC PC
#endif

typedef struct {                       /* stands for a SEQAIJ Mat: host CSR view */
  int n;                               /* rows = cols */
  const int* rowptr;                   /* n + 1 */
  const int* col;                      /* rowptr[n], local indices, ascending per row */
  const double* val;
} GeneoCsr;

typedef struct {                       /* stands for an IS: host index list */
  int n;
  const int* idx;
} GeneoIS;

typedef struct {                       /* stands for the MATIS operator (driver:755-757) */
  int nbDOF;                           /* global size N */
  int nbDOFLoc;                        /* local size */
  const int* map;                      /* local -> global, ascending (driver:1292-1298) */
  GeneoCsr local;                      /* local (Neumann) matrix, MatISGetLocalMat */
} GeneoMatIS;

/* ---- lifecycle ------------------------------------------------------------------------- */
/* PCCreate + PCSetType(pc,"geneo"): allocates the PC shell, then calls createGenEOPC on it. */
PetscErrorCode PCCreate_GenEO(GENEO_PC* pc);
/* src/geneo.cpp:2639-2728: (re)creates the context with the reference's default parameters. */
#ifndef GENEO_HAVE_PETSC
PetscErrorCode createGenEOPC(GENEO_PC pc);
#endif
/* The same entry under a name of its own.  A PETSc-side adapter defines the reference's createGenEOPC(PC) and
 * PCGenEOSetup(PC, Mat, IS, IS*) with PETSc's types (that is what the reference's driver links against) and forwards
 * to these two; with GENEO_HAVE_PETSC the header therefore does not declare the reference-named pair. */
PetscErrorCode PCGenEOCreateContext(GENEO_PC pc);
/* src/geneo.cpp:2180-2243 */
PetscErrorCode PCDestroy_GenEO(GENEO_PC* pc);

/* ---- options (src/geneo.cpp:2329-2514) -------------------------------------------------- */
/* Parses the -geneo_* options (same spellings, defaults, validation), plus the subset of the
 * forwarded prefixes this build understands: -els2_eps_{tol,nev,max_it,block,seed},
 * -els2_cheb_{degree,ratio}, -dls1_ksp_{type,rtol,max_it}, -ksp_{type,rtol,atol,divtol,max_it},
 * -ksp_gmres_restart.  Unknown options are ignored, like PETSc with -options_left no.
 * -dls1_ksp_type cg|chebyshev (default cg) chooses the Krylov method of the local solves: the batched V-cycle-PCG run to
 * -dls1_ksp_rtol, or a fixed-degree Chebyshev iteration preconditioned by the same V-cycle (needs -dls1_pc_type amg; any
 * other value is refused).  Chebyshev has no reductions and no host polling and is a fixed linear operator at any
 * -dls1_ksp_rtol; per subdomain its bounds come from -dls1_cheb_esteig_its Lanczos steps (default 16) scaled by
 * -dls1_cheb_safety lo,hi (default 0.9,1.1), and its degree is the smallest k with 1 / T_k(sigma) <= -dls1_ksp_rtol,
 * at most -dls1_ksp_max_it.  With chebyshev both are read by the set-up, which fixes the degrees: changing them with
 * PCGenEOSetOption afterwards has no effect before the next set-up (the cg path reads them at every solve).  A degree cut
 * short by -dls1_ksp_max_it is no error here (the cg path raises KSP_DIVERGED_ITS): the operator stays linear, symmetric and
 * positive definite, only less accurate, and PCGenEOGetLocalSolverInfo reports the degree and the reduction reached. */
PetscErrorCode PCSetFromOptions_GenEO(GENEO_PC pc, int argc, const char* const* argv);
PetscErrorCode PCGenEOSetOption(GENEO_PC pc, const char* key, const char* value);
/* buildGenEOName, src/geneo.cpp:2245-2268 ("geneo1ASM", "geneo1HASM", ...) */
const char* PCGenEOGetName(GENEO_PC pc);
const char* PCGenEOGetError(GENEO_PC pc);
/* the parsed options as "key=value;..." (what the driver reads from the public geneoContext fields,
 * src/geneo4PETSc.cpp:928-989) */
const char* PCGenEOGetOptionsString(GENEO_PC pc);
/* usageGenEO, src/geneo.cpp:2274-2327 */
const char* usageGenEO_c(void);

/* ---- inputs ----------------------------------------------------------------------------- */
/* KSPSetOperators(ksp, A, A) with A of type MATIS (required: src/geneo.cpp:1681). */
PetscErrorCode PCSetOperators_GenEO(GENEO_PC pc, const GeneoMatIS* A);
/* hdr/geneo_c.h:10, src/geneo.cpp:2518-2572: one subdomain per rank, operator taken from
 * PCSetOperators_GenEO; pcADirLoc may be NULL (built from A); dofIntersections may be NULL
 * (only its emptiness pattern is used, and only by GenEO-2). */
#ifndef GENEO_HAVE_PETSC
PetscErrorCode PCGenEOSetup(GENEO_PC pc, const GeneoCsr* pcADirLoc, GeneoIS dofMultiplicities,
                            const GeneoIS* dofIntersections);
#endif
PetscErrorCode PCGenEOSetupViews(GENEO_PC pc, const GeneoCsr* pcADirLoc, GeneoIS dofMultiplicities,
                                 const GeneoIS* dofIntersections);   /* = PCGenEOSetup, see PCGenEOCreateContext */
/* C form of initGenEOPC (hdr/geneo.hpp:30-35, src/geneo.cpp:2591-2632). b_dev / x0_dev may be NULL. */
PetscErrorCode initGenEOPC_c(GENEO_PC pc, unsigned int nbDOF, unsigned int nbDOFLoc, const int* map,
                             const GeneoCsr* A_local, const GeneoCsr* ADirLoc, const double* b_dev,
                             double* x0_dev, const unsigned int* dofIdxMultLoc);

/* Several subdomains on one rank / GPU (extension; gid = the MPI rank the reference would use). */
PetscErrorCode PCGenEOSetSizes(GENEO_PC pc, int nbDOF, int nbSubdomainsGlobal);
PetscErrorCode PCGenEOAddSubdomain(GENEO_PC pc, int gid, int nbDOFLoc, const int* map, const int* multiplicity,
                                   const GeneoCsr* A_local, const GeneoCsr* ADirLoc);

/* intersectLoc of initGenEOPC (hdr/geneo.hpp:34): nonempty[q] != 0 iff subdomain gid shares DOFs with
 * subdomain q.  Only GenEO-2's gamma_loc reads it (src/geneo.cpp:1139-1148); on one rank it is derived
 * from the maps when absent.  gid < 0 addresses the subdomain added last. */
PetscErrorCode PCGenEOSetIntersect(GENEO_PC pc, int gid, int nbSubdomainsGlobal, const int* nonempty);

/* ---- multi-rank plumbing (one process per GPU; the transport is supplied by the host) ----- */
typedef int (*GeneoExchangeFn)(void* user, int reverse);  /* 0 = forward (owner -> halo), 1 = reverse */
typedef int (*GeneoAllreduceFn)(void* user, int n);       /* in-place sum of red_dev[0..n) over ranks */
/* owned_gid: ascending global ids owned by this rank.  halo_gid: ids this rank reads but does not
 * own, grouped by owner rank (recv_counts[q] ids from rank q).  send_idx: owned-local indices this
 * rank sends, grouped by destination (send_counts[q]).  The callbacks move send_dev -> recv_dev
 * with these counts (forward) or with the two count arrays swapped (reverse), on the stream given
 * to GeneoSetStream.  Buffers are device memory owned by the caller (>= max(sum send, sum recv)). */
PetscErrorCode PCGenEOSetComm(GENEO_PC pc, int rank, int size, int n_owned, const int* owned_gid, int n_halo,
                              const int* halo_gid, const int* recv_counts, const int* send_counts,
                              const int* send_idx, GeneoExchangeFn exchange, GeneoAllreduceFn allreduce,
                              void* user, double* send_dev, double* recv_dev, double* red_dev, int red_capacity);
/* Optional: send_dev / recv_dev hold max_width x the single-vector counts (entry-major, the vectors of one entry
 * contiguous) and the exchange callback honours the width passed in the upper bits of its flag
 * (flag = reverse | width << 1; width 0 means 1).  Lets the coarse operator E be assembled 32 columns per
 * exchange instead of one.  Default width 1. */
PetscErrorCode PCGenEOSetCommWidth(GENEO_PC pc, int max_width);

/* C++ transport over RCCL / xGMI built into the library (csrc/comm_rccl.cpp): the counterpart of the reference's
 * VecScatter (src/geneo.cpp:156,:1850,:1881) and MPI reductions (:1474) for one process per GPU.  Halo exchanges are
 * ncclSend / ncclRecv groups with the neighbours, reductions ncclAllReduce, all on the stream given to GeneoSetStream.
 * Bootstrap: rank 0 calls GeneoRcclUniqueId and the HOST broadcasts the 128 bytes (MPI_Bcast, torch.distributed, ...);
 * every rank then calls GeneoRcclCreate (collective) and attaches its PCs with PCGenEOSetCommRccl, which allocates the
 * device buffers (max_width vectors per exchange, cf. PCGenEOSetCommWidth) and installs the two callbacks of
 * PCGenEOSetComm.  RCCL is resolved with dlopen: no link-time dependency. */
typedef struct _p_GeneoRccl* GeneoRccl;
PetscErrorCode GeneoRcclUniqueId(char* id128);
PetscErrorCode GeneoRcclCreate(const char* id128, int rank, int size, GeneoRccl* comm);
PetscErrorCode PCGenEOSetCommRccl(GENEO_PC pc, GeneoRccl comm, int n_owned, const int* owned_gid, int n_halo,
                                  const int* halo_gid, const int* recv_counts, const int* send_counts,
                                  const int* send_idx, int max_width);
PetscErrorCode GeneoRcclDestroy(GeneoRccl* comm);
const char* GeneoRcclGetError(void);
/* bring-up hooks: the device buffers of the which-th attached plan and direct calls of its two callbacks */
PetscErrorCode GeneoRcclPlanBuffers(GeneoRccl comm, int which, double** send_dev, double** recv_dev, double** red_dev);
PetscErrorCode GeneoRcclPlanExchange(GeneoRccl comm, int which, int flag);
PetscErrorCode GeneoRcclPlanAllreduce(GeneoRccl comm, int which, int n);

/* ---- PC operations (the PETSc ops table, src/geneo.cpp:2717-2720) ------------------------- */
PetscErrorCode PCSetUp_GenEO(GENEO_PC pc);                                   /* setUpGenEOPC :1672 */
PetscErrorCode PCApply_GenEO(GENEO_PC pc, const double* x_dev, double* y_dev); /* applyGenEOPC :2051 */
PetscErrorCode PCGenEOApplyQ(GENEO_PC pc, const double* x_dev, double* y_dev); /* applyQ :1435 */
PetscErrorCode MatMult_GenEO(GENEO_PC pc, const double* x_dev, double* y_dev); /* MatMult on the MATIS A */
/* initial guess written by setup (src/geneo.cpp:1601-1607): Q b for the efficient hybrid, else 0 */
PetscErrorCode PCGenEOGetX0(GENEO_PC pc, double* x0_dev);
PetscErrorCode PCGenEOSetRHS(GENEO_PC pc, const double* b_dev);

/* ---- Krylov driver (counterpart of KSPSolve at src/geneo4PETSc.cpp:1240; PETSc's own KSP
 *      drives PCApply_GenEO instead when PETSc is present) ----------------------------------- */
PetscErrorCode KSPSolve_GenEO(GENEO_PC pc, const double* b_dev, double* x_dev, int* its, double* rnorm, int* reason);
int PCGenEOGetResidualHistory(GENEO_PC pc, double* hist, int cap);
/* -ksp_type cg|gmres|fgmres|fcg (fcg: below) and -ksp_pc_side left|right (default left) choose the method of KSPSolve_GenEO.  cg and gmres are
 * left-preconditioned: their convergence test, rnorm and residual history are those of the preconditioned residual.
 * -ksp_type gmres -ksp_pc_side right is restarted GMRES on A M^-1; -ksp_type fgmres is flexible GMRES, always right, which
 * keeps z_k = M^-1 v_k of every step and so allows a preconditioner that changes between applications (-dls1_ksp_type cg at
 * a loose -dls1_ksp_rtol).  Both test, report and record the norm of the TRUE residual b - A x: r_0 is recomputed at every
 * restart, and with -ksp_initial_guess_nonzero the test is relative to |b|, as KSPConvergedDefault does.  Classical
 * Gram-Schmidt: a step takes all its coefficients from one pass over the basis and one all-reduce of k + 1 values, and the
 * projection with the norm of the remainder from a second pass and an all-reduce of one.  reason -5
 * (KSP_DIVERGED_BREAKDOWN) reports a zero rotation.  The basis (restart + 1 vectors; twice that for fgmres) is allocated by
 * the first such solve, grown as the steps need it, kept for the next solve and freed with the set-up: a PC that never runs
 * one pays nothing.
 * Refused: -ksp_type cg with -ksp_pc_side right, -ksp_type fgmres with -ksp_pc_side left and any other side, when the option
 * is set; either method with -geneo_lvl ...,E1 | E2, at the solve (the projected operator and the initial guess of the
 * efficient hybrid are argued for left preconditioning); KSPMatSolve_GenEO with -ksp_pc_side right.  PETSc's own KSP needs
 * nothing from the PC for -ksp_pc_side right or -ksp_type fgmres: this is the stand-alone driver's counterpart.
 * PCGenEOGetKrylovInfo: *basis_vectors device vectors these methods hold now (basis, flexible basis and scratch) and
 * *basis_bytes their bytes with the pointer tables, coefficients and partial sums (both 0 before the first such solve of a
 * set-up); since the set-up the Gram-Schmidt passes through the fused kernels, *gs_fused, and through their composed forms,
 * *gs_composed (GeneoSetKernelVariant("krylov_fused", 0), or a backend without the kernels); and the applications of the
 * preconditioner, *pc_applies, and the operator products, *mat_mults, of the last KSPSolve_GenEO, whatever its method.
 * Any pointer may be NULL.  Returns 0, -1 for a bad handle. */
int PCGenEOGetKrylovInfo(GENEO_PC pc, int* basis_vectors, double* basis_bytes, long long* gs_fused, long long* gs_composed,
                         long long* pc_applies, long long* mat_mults);
/* -ksp_type fcg is the flexible CG of Notay (PETSc KSPFCG): left-preconditioned like cg, with cg's norms and short
 * recurrences, for the symmetric modes (ASM, SRAS, SORAS and their hybrids) under a preconditioner that changes between
 * applications.  A new direction is made conjugate to the m_i = min(i, mi) most recent ones, mi = max(1, i mod (mmax + 1))
 * (-ksp_fcg_truncation_type notay, the default) or mi = mmax (standard), -ksp_fcg_mmax mmax >= 1 (default 30); mmax + 1
 * directions and their products are held at most, each allocated when a step first needs it, all freed with the set-up.
 * Per iteration one pass gives the window's dot products and (z, z), one all-reduce and ONE download follow; the step
 * x += alpha p, r -= alpha A p takes alpha = (r, p) / (A p, p) from the device.  (A p, p) <= 0 leaves x and r untouched
 * and is reported as KSP_DIVERGED_INDEFINITE_MAT (-8) with the its of that iteration.
 * -ksp_norm_type preconditioned|unpreconditioned (default preconditioned): unpreconditioned tests, reports and records
 * |b - A x|, relative to |b| with -ksp_initial_guess_nonzero; it is accepted with fcg only -- KSPSolve_GenEO with any other
 * -ksp_type, and KSPMatSolve_GenEO, refuse it.  -ksp_pc_side right with fcg is refused when either option is set;
 * KSPMatSolve_GenEO has no block form of it.
 * PCGenEOGetFcgInfo: *directions direction / product pairs held now and *bytes the device bytes of everything the method
 * holds (both 0 before the first fcg solve of a set-up); since the set-up the steps through the fused kernel, *steps_fused,
 * and through its composed form, *steps_composed (GeneoSetKernelVariant("krylov_fused", 0), or a backend without the
 * kernel); of the last fcg solve the largest window, *max_window, and the device-to-host copies the host waited for,
 * *downloads.  PCGenEOGetKrylovInfo's *pc_applies and *mat_mults count an fcg solve too; its other fields do not.
 * Any pointer may be NULL.  Returns 0, -1 for a bad handle. */
int PCGenEOGetFcgInfo(GENEO_PC pc, int* directions, double* bytes, long long* steps_fused, long long* steps_composed,
                      int* max_window, long long* downloads);

/* ---- blocks of right-hand sides (-geneo_block_width 16 | 32; needs -dls1_ksp_type chebyshev) --------------------------
 * The counterparts of pc->ops->matapply, MatMatMult on the MATIS operator and KSPMatSolve.  Blocks are column-major with a
 * leading dimension, as PETSc's MatDense holds them: n_owned rows, m >= 1 columns, ld >= n_owned, device memory.  Columns
 * are processed in slabs of the width; the last slab is padded with zero columns, which stay exactly zero through every
 * linear step and are never written back.  Bytes of the output beyond column m and between row n_owned and ld are not
 * touched.
 * The local solve of a slab is the fixed chain of launches of the Chebyshev local solver with SpMM in place of SpMV,
 * replayed from a HIP graph of its own.  Its V-cycle reads the FP64 level matrices: under -dls1_amg_precision single the
 * single-vector path reads their float companions and the two are slightly different (fixed, linear, symmetric)
 * operators; under -dls1_amg_precision double they differ by summation order alone.
 * KSPMatSolve_GenEO: preconditioned CG on every column in lock step with a zero initial guess (X is zeroed by the library);
 * every column runs its own convergence test and is frozen once it has met it.  its / rnorm / reason: m entries each, host.
 * -ksp_matsolve_type cg|gmres chooses the Krylov method of KSPMatSolve_GenEO alone.  Unset, the method is -ksp_type, which
 * must then be cg: -ksp_type gmres on its own is refused.  gmres is KSPSolve_GenEO's restarted GMRES (left preconditioning,
 * classical Gram-Schmidt, Givens residual; -ksp_gmres_restart, -ksp_rtol / atol / divtol / max_it as there) on every column
 * in lock step, for the non-symmetric modes (RAS, ORAS, the hybrid ones): the columns share the step index and the restart
 * boundary, each has its own Hessenberg system and test, and a column that met its test is frozen -- its basis columns are
 * exact zeros from then on.  A step takes all its Gram-Schmidt coefficients from one pass over the basis and one all-reduce
 * of (k + 1) w values, and the projection with the norms of the remainder from a second pass and an all-reduce of w.  The
 * basis (restart + 1 slabs at most) is allocated by the first such solve, grown as the steps need it, kept for the next
 * solve and freed with the set-up: a PC that never runs one pays nothing.
 * -ksp_initial_guess_nonzero (the default of this library: pass -ksp_initial_guess_nonzero 0) is refused by both
 * methods.  PCGenEOGetResidualHistory is not extended to blocks.
 * Each returns an error, not a crash, for a set-up without -geneo_block_width, a PC that is not set up, ld < n_owned and
 * m < 1.  The width is read by the set-up: changing the option afterwards has no effect before the next set-up. */
PetscErrorCode PCMatApply_GenEO(GENEO_PC pc, const double* X_dev, int ldx, double* Y_dev, int ldy, int m);
PetscErrorCode MatMatMult_GenEO(GENEO_PC pc, const double* X_dev, int ldx, double* Y_dev, int ldy, int m);
PetscErrorCode KSPMatSolve_GenEO(GENEO_PC pc, const double* B_dev, int ldb, double* X_dev, int ldx, int m, int* its,
                                 double* rnorm, int* reason);
/* Since the set-up: the width, the slabs that went through the block apply (KSPMatSolve_GenEO's included), their columns,
 * the zero columns that padded them, and the local solves of slabs replayed from the HIP graph (the others went out as
 * direct launches: the first one, one in eight while the in-situ kernel timer runs, and all of them where capture is
 * unavailable).  Any pointer may be NULL.  Returns 0, -1 for a bad handle. */
int PCGenEOGetBlockInfo(GENEO_PC pc, int* width, long long* slabs, long long* columns, long long* padded,
                        long long* graph_launches);
/* Block GMRES (-ksp_matsolve_type gmres): *basis_slabs basis slabs held now and *basis_bytes the device bytes of the basis
 * with its pointer table, coefficients and partial sums (both 0 before the first block GMRES solve of a set-up), and since
 * the set-up the Gram-Schmidt passes (one for the dots and one for the update of every step, one for the solution update
 * of every cycle) that went through the fused kernels, *gs_fused, and through their composed forms, *gs_composed
 * (GeneoSetKernelVariant("block_fused", 0), or a backend without the kernels).  Read-only; any pointer may be NULL.
 * Returns 0, -1 for a bad handle. */
int PCGenEOGetBlockKrylovInfo(GENEO_PC pc, int* basis_slabs, double* basis_bytes, long long* gs_fused,
                              long long* gs_composed);
/* Since the set-up: how the slabs of the block apply had E^-1 applied to their dimE x w coarse block -- *blocked by the
 * blocked device sweeps on the whole block (a factor made on the device: the launches of one single-vector sweep pair for
 * all w columns), *by_column column by column through the single-vector path (GeneoSetKernelVariant("block_fused", 0), or
 * a backend without the block kernel), *host_blocks by one download, w host solves and one upload (a factor held on the
 * host).  Slabs that took the one-launch kernel of a host-made factor on the device (dimE <= 1024) are in none of the
 * three.  Any pointer may be NULL.  Returns 0, -1 for a bad handle. */
int PCGenEOGetCoarseBlockCounters(GENEO_PC pc, long long* blocked, long long* by_column, long long* host_blocks);

/* ---- public counters / timers of geneoContext (hdr/geneo.hpp:96-123) ----------------------- */
typedef struct {
  int estimDimELoc, realDimELoc, nicolaidesLoc, dimE;
  int eig_iterations, eig_spmm;
  long long dls1_iterations, dls1_solves, spmv_calls;
  double lvl1SetupMinvTimeLoc, lvl2SetupEigTimeLoc, lvl2SetupZTimeLoc, lvl2SetupETimeLoc;
  double lvl1ApplyTimeLoc, lvl1ApplyScatterTimeLoc, lvl1ApplyMinvTimeLoc, lvl1ApplyGatherTimeLoc;
  double lvl1ApplyPrjFSTimeLoc, lvl2ApplyTimeLoc, lvl2ApplyZtTimeLoc, lvl2ApplyEinvTimeLoc, lvl2ApplyZTimeLoc;
  double setupTime, solveTime;
  int amg_levels;                       /* levels of the inner AMG hierarchy (0 = not used) */
  double amg_operator_complexity, amgSetupTime;
  int nullPivotsLoc;                    /* null pivots detected and fixed in the local factorisations of this set-up (singular
                                           subdomain matrices; the reference's MUMPS settings of tuneSolver, geneo.cpp:76-92) */
  int eigGroups;                        /* consecutive subdomain groups the local eigensolves of this set-up ran in (1: all at once;
                                           > 1: memory-bounded set-up, -geneo_eig_group_rows / -geneo_eig_mem_gb) */
  int eigCoarseIterations;              /* LOBPCG iterations spent on the multigrid level-1 pencil whose Ritz vectors start the fine
                                           eigensolve (-geneo_eig_coarse_start; 0: the fine eigensolve started from its random block) */
} GeneoInfo;
PetscErrorCode PCGenEOGetInfo(GENEO_PC pc, GeneoInfo* info);
/* eigenvalues kept in Z for local subdomain s (returns the count; copies min(count, cap)) */
int PCGenEOGetEigenvalues(GENEO_PC pc, int local_sub, double* vals, int cap);
int PCGenEOGetCandidates(GENEO_PC pc, int local_sub, double* vals, int cap);
/* coarse operator E (dimE x dimE row-major); returns dimE */
int PCGenEOGetE(GENEO_PC pc, double* e, int cap);
int PCGenEOGetLocalDims(GENEO_PC pc, int* ksub_global, int cap);
/* tau_loc / gamma_loc per local subdomain (getLocalGenEOTau / Gamma, src/geneo.cpp:1097-1232); returns the count */
int PCGenEOGetLocalParams(GENEO_PC pc, double* tau_loc, double* gamma_loc, int cap);

/* ---- input plugins ------------------------------------------------------------------------------
 * The reference driver loads its operators from `--inpLibA lib.so#args` plugins exporting the C++ function
 * `getInput` (src/geneo4PETSc.cpp:75-96; tst/laplacian, tst/heat, tst/graph).  GeneoGetLibInput loads such a
 * plugin unchanged ('#' in the arguments stands for a blank, as on the reference CLI) and returns the element
 * list flattened: element e has nodes elemIdx[elemPtr[e] .. elemPtr[e+1]) and a row-major k x k matrix, the
 * matrices stored back to back in elemMat.  Free with GeneoFreeInput. */
typedef struct {
  unsigned int nbElem, nbNode;
  unsigned int* elemPtr;   /* nbElem + 1 */
  unsigned int* elemIdx;   /* nIdx */
  double* elemMat;         /* nMat */
  size_t nIdx, nMat;
} GeneoInput;
PetscErrorCode GeneoGetLibInput(const char* inpLibA, const char* inpLibArg, GeneoInput* out);
void GeneoFreeInput(GeneoInput* in);

/* ---- host-side decomposition and structured generators (csrc/decompose.cpp) ---------------------------------------
 * The reference DRIVER's decompose + addOverlapLayers + buildDomain + fillALoc (src/geneo4PETSc.cpp:196-379, :447-494,
 * :643-715): from the element lists and a k-way partition (elemPart when dual, nodePart when nodal) to each domain's
 * ascending global node list, multiplicities, MATIS local matrix A_Neu (element matrices weighted 1 / elemMult) and
 * A_Dir = R A R^T, plus the lists of local indices shared with every other domain (intersectLoc, hdr/geneo.hpp:34).
 * nodes: nbElem x W node ids (-1: unused slot), mats: nbElem x W*W; both must outlive the handle.  GeneoDomain arrays
 * are malloc'ed by the library: release with GeneoFreeDomain.  Host code only. */
typedef struct _p_GeneoDecomp* GeneoDecomp;
typedef struct {
  int n;                                /* local DOFs */
  int *l2g, *mult;                      /* n each */
  int *neu_rowptr, *neu_col; double* neu_val;
  int *dir_rowptr, *dir_col; double* dir_val;     /* NULL without withDirichlet */
  int *inter_ptr, *inter_idx;           /* nbPart + 1 offsets into the shared local indices, per other part */
} GeneoDomain;
PetscErrorCode GeneoDecompCreate(int nbNode, int nbElem, int W, const int* nodes, const double* mats, int nbPart,
                                 const int* elemPart, const int* nodePart, int dual, int addOverlap, GeneoDecomp* out);
PetscErrorCode GeneoDecompDomain(GeneoDecomp d, int p, int withDirichlet, GeneoDomain* out);
void GeneoFreeDomain(GeneoDomain* dom);
void GeneoDecompDestroy(GeneoDecomp* d);
/* tst/laplacian (laplacian.cpp:57-188) / tst/heat (heat.cpp:64-261) generator on an n^dim grid (interp: 0 none, 1 quad,
 * 2 lin, 3 minmax), optionally restricted to the elements inside the node-index box [wlo, whi) (NULL: whole grid).
 * nodes (nbElem x 2, -1 in the second slot of a Dirichlet element) and mats (nbElem x 4) are malloc'ed: GeneoFreeMesh. */
PetscErrorCode GeneoGridMesh(int n, int dim, double inpEps, double kappaMax, int interp, int heat, double lbd, double dt,
                             const int* wlo, const int* whi, int* nbNode, int* nbElem, int** nodes, double** mats);
void GeneoFreeMesh(int* nodes, double* mats);

/* ---- host k-way mesh partitioner (csrc/partition.cpp): what the reference's driver asks of Metis 5.1.0 --------------
 * METIS_PartMeshDual(&ne, &nn, eptr, eind, NULL, NULL, &ncommon = 1, &nparts, NULL, options, &objval, epart, npart) and
 * METIS_PartMeshNodal(&ne, &nn, eptr, eind, NULL, NULL, &nparts, NULL, options, &objval, epart, npart) with
 * PTYPE_KWAY / OBJTYPE_CUT (src/geneo4PETSc.cpp:381-445).  Elements are node lists (eptr[ne + 1], eind[eptr[ne]]);
 * epart[ne] / npart[nn] receive the parts; objval the edge cut of the partitioned graph.  Multilevel recursive bisection
 * (heavy-edge matching, graph growing + spectral initial cuts, FM refinement, multilevel spectral candidate); sizes exact
 * to one vertex per bisection; deterministic.  Host code only (no device is touched).  0 = ok. */
int GeneoPartMeshDual(int ne, int nn, const int* eptr, const int* eind, int nparts, int* objval, int* epart, int* npart);
int GeneoPartMeshNodal(int ne, int nn, const int* eptr, const int* eind, int nparts, int* objval, int* epart, int* npart);
/* METIS_PartGraphKway on a CSR graph (symmetric adjacency, no self loops, unit weights) */
int GeneoPartGraphKway(int n, const int* xadj, const int* adjncy, int nparts, int* objval, int* part);

/* ---- the CLI driver (csrc/driver_main.cpp): counterpart of the reference executable's main() (src/geneo4PETSc.cpp:1569)
 * with its flags (--inpFileA / --inpLibA / --inpFileB / --inpEps / --metisDual / --metisNodal / --addOverlap / --verbose /
 * --timing / --shortRes / --cmdLine; --np N for `mpirun -n N`, --parts / --partFile for a given partition; everything else
 * goes to the PC) and its INFO: / TIME: output lines (driver:898-1231) on stdout.  argv WITHOUT the program name.
 * The executable geneo4petsc_amd/geneo_driver is a main() over it.  0 = ok. */
int GeneoDriverMain(int argc, const char* const* argv);

/* ---- device helpers for hosts without a HIP runtime of their own ---------------------------- */
const char* GeneoBackendName(void);              /* "hip-gfx950" in the product library */
PetscErrorCode GeneoSetStream(void* hip_stream); /* all launches / copies go to this stream */
/* One process per GPU: bind this process to GPU (local_rank mod GeneoDeviceCount()) BEFORE the first allocation, set-up
 * or RCCL call (ncclCommInitRank refuses two ranks on one device).  Returns the device ordinal, -1 on failure.  The
 * reference has no counterpart (CPU only); under mpirun pass the rank inside the node (MPI_Comm_split_type(SHARED)),
 * as adapters/geneo_petsc_adapter.cpp does -- or give every rank its own HIP_VISIBLE_DEVICES and skip the call. */
int GeneoDeviceCount(void);
int GeneoSetDevice(int local_rank);
/* The HIP current device belongs to the host THREAD: the library binds every thread it starts (side-stream set-up, upload
 * helpers) to the device of the thread that configured it (GeneoSetDevice, GeneoSetStream or the first allocation).
 * GeneoCurrentDevice: that device (-1 before the first call).  GeneoThreadDeviceCheck (test hook): starts a thread the
 * way the library does and returns the device it ends up on -- equal to GeneoCurrentDevice() or the binding is broken. */
int GeneoCurrentDevice(void);
int GeneoThreadDeviceCheck(void);
/* hipFree every device block the library's caching allocator is holding (it keeps freed blocks for the next set-up, up
 * to GENEO_ALLOC_CACHE_GB, default 96): call it when another allocator of the process needs the memory. */
void GeneoAllocCacheRelease(void);
void* GeneoDeviceAlloc(size_t bytes);
void GeneoDeviceFree(void* p);
PetscErrorCode GeneoH2D(void* dst_dev, const void* src, size_t bytes);
PetscErrorCode GeneoD2H(void* dst, const void* src_dev, size_t bytes);
PetscErrorCode GeneoDeviceSync(void);
int GeneoSelfTestMFMA(void);                     /* 0 = f64 MFMA lane maps as assumed */
/* y = a x + b y on device vectors (calibration kernel of the HBM-traffic PMC passes) */
PetscErrorCode GeneoTestAxpby(double* y_dev, const double* x_dev, double a, double b, int n);
PetscErrorCode GeneoSetSpmvKind(int kind);       /* 0: LDS row-block SpMV kernel, 1: 64-row sliced kernel (default) */
const char* GeneoSpmvKernelName(void);
PetscErrorCode GeneoSetMFMA(int enable);         /* 0: run the plain-FMA twins of the MFMA kernels (validation) */
/* validation: choose between two device forms of the same arithmetic -- "spgemm_fill_scan" (1: owner-computes numeric pass
 * of the sparse products instead of the hash accumulators), "spgemm_small_rows" (0: rows of at most 64 products go through
 * the hash table as well), "gram_flat" (0: k_gram_mfma instead of k_gram_flat); both forms of each give bit-identical
 * results (tests/test_gpu_kernels.py).  "cheb_fused" (0: the step of the Chebyshev local solver composed of the plain
 * vector primitives and its residual update as the plain product and a vector update, instead of their fused kernels;
 * same bits).  "block_fused" (0: the operations of the block entry points composed of the plain primitives instead of
 * the kernels of csrc/block_dev.h; same bits in PCMatApply_GenEO).  Returns 1 for an unknown name. */
PetscErrorCode GeneoSetKernelVariant(const char* name, int value);

/* ---- stand-alone kernels (parity tests and the roofline leg of bench.py) --------------------- */
typedef struct _p_GeneoSpmv* GeneoSpmv;
PetscErrorCode GeneoSpmvCreate(const GeneoCsr* a, GeneoSpmv* h);
PetscErrorCode GeneoSpmvApply(GeneoSpmv h, const double* x_dev, double* y_dev);
/* average kernel time of `reps` back-to-back launches, HIP events on the library stream */
PetscErrorCode GeneoSpmvTime(GeneoSpmv h, const double* x_dev, double* y_dev, int reps, double* ms_avg);
PetscErrorCode GeneoSpmvDestroy(GeneoSpmv* h);
/* in-situ timing of every `every`-th CSR SpMV launch the library issues (solve loops included):
 * HIP events on the launch stream; stop returns the summed kernel ms and algorithmic bytes. */
PetscErrorCode GeneoSpmvProfileStart(int every, double min_bytes);  /* launches moving < min_bytes are skipped */
PetscErrorCode GeneoSpmvProfileStop(double* ms_sum, double* bytes_sum, long long* nsampled, long long* nlaunch);
/* the same for every hot kernel class at once: 0 fine-level CSR SpMV, 1 fine-level SpMM (16 / 32 / 64 columns),
 * 2 MFMA Gram (S^T T), 3 MFMA block update (S C).  Start ... the library's work ... Stop, then Get per class: summed
 * kernel ms, algorithmic bytes and flops of the SAMPLED launches, their number and the number of launches seen. */
PetscErrorCode GeneoKernelProfileStart(int every, double spmv_min_bytes);
/* Device memory of the library's own blocks, in bytes (any pointer may be NULL): handed out now, their high-water mark,
 * the high-water mark of handed out + parked in the caching allocator (the library's footprint on the card), parked now,
 * and hipMemGetInfo's free / total.  reset_peaks != 0 restarts both high-water marks at the current state. */
PetscErrorCode GeneoDeviceMemInfo(double* live, double* live_peak, double* footprint_peak, double* cached, double* dev_free,
                                  double* dev_total, int reset_peaks);
PetscErrorCode GeneoKernelProfileStop(void);
PetscErrorCode GeneoKernelProfileGet(int kernel_class, double* ms_sum, double* bytes_sum, double* flops_sum,
                                     long long* nsampled, long long* nlaunch);
/* Y = post.*(A (pre.*X)), row-major n x m blocks */
PetscErrorCode GeneoSpmmApply(GeneoSpmv h, const double* X_dev, double* Y_dev, int m, const double* pre_dev,
                              const double* post_dev);
/* the same on strided blocks (leading dimensions ldx / ldy >= m), timed: average kernel time of `reps` back-to-back
 * launches, HIP events on the library stream (reps <= 0: one untimed launch, ms_avg untouched) */
PetscErrorCode GeneoSpmmTime(GeneoSpmv h, const double* X_dev, int ldx, double* Y_dev, int ldy, int m,
                             const double* pre_dev, const double* post_dev, int reps, double* ms_avg);
/* multigrid epilogues fused into the SpMV (m = 1) / SpMM launch, row-major n x m blocks:
 *   epi 1: Y = B - A X      2: Y = Z + A X      3: Y = X + w dinv.*(B - A X)      4: Z = w dinv.*B, Y = B - A Z
 *   epi 5: Y = w dinv.*(Z + B) + A X (prolongation + correction + post-smoothing sweep in one product) */
PetscErrorCode GeneoSpmmFused(GeneoSpmv h, int epi, const double* X_dev, double* Y_dev, int m, const double* B_dev,
                              double* Z_dev, const double* dinv_dev, double w);
/* the single-vector launches (m = 1; epi 0: Y = A X) reading the matrix's single-precision companion -- float values,
 * 16-bit column offsets per 64-row slice (32-bit columns when a slice spans more than 65535), FP64 arithmetic: what the V-cycle of the local solves streams
 * (-dls1_amg_precision single).  Error when the matrix has no such companion. */
/* Y1 = B X, Y2 = A X in ONE pass over X with B laid out on A's sliced pattern (LOBPCG's A W / B W pass); 2 = pattern(B)
 * not contained in pattern(A) or A not on the sliced path */
PetscErrorCode GeneoSpmmDualTest(GeneoSpmv a, GeneoSpmv b, const double* X_dev, int ldx, double* Y1_dev, double* Y2_dev,
                                 int ldy, int m);
/* R = mask .* (A X - B X diag(lam)) per subdomain, both products in one pass over X and neither written (the residual
 * block of LOBPCG's lean iteration); suboff: nsub + 1 first rows, lam / mask: nsub x m HOST arrays; X_dev, R_dev device */
PetscErrorCode GeneoSpmmDualResidualTest(GeneoSpmv a, GeneoSpmv b, const double* X_dev, int ldx, double* R_dev, int ldr,
                                         int m, int nsub, const int* suboff, const double* lam, const double* mask);
PetscErrorCode GeneoSpmvFusedSingle(GeneoSpmv h, int epi, const double* X_dev, double* Y_dev, const double* B_dev,
                                    double* Z_dev, const double* dinv_dev, double w);
/* what the offset coding of the columns found on the matrix (made with the single-precision companion, i.e. by the first
 * GeneoSpmvFusedSingle): its 64-row slices, and how many of them are coded (0 on a backend without the coded kernels) */
PetscErrorCode GeneoSpmvOffsetInfo(GeneoSpmv h, int* slices, int* coded);
/* device sparse products of the multigrid set-up (test hook): op 0: C = A B, op 1: C = A^T; returns nnz(C), -1 when a
 * row exceeds the kernels' per-row capacity (callers fall back to the host product), -2 on error */
long long GeneoTestSparseProduct(int op, const GeneoCsr* A, const GeneoCsr* B, int ncols, int* rowptr_out, int* col_out,
                                 double* val_out, long long cap);
/* what the calling thread's last device sparse product decided (test hook): *group the lanes per row of the short-row
 * pass (0: none, 8, 16, 32, 64), *deferred the rows that pass left to the wave-per-row kernels, *scan_depth how the row
 * pointers were scanned (0: host loop, 1: one level of block totals, 2: the totals scanned in more than one block).
 * A backend without these paths reports zeros.  Any pointer may be NULL.  Returns 0. */
int GeneoTestSparseProductReport(int* group, int* deferred, int* scan_depth);
/* per-subdomain tall-skinny kernels on host data (suboff: nsub+1 row offsets):
 *   kind 0: G[s] = S_s^T T_s (p x q)     kind 1: Y_s = S_s C_s (C: nsub x p x q)
 *   kind 2: kind 0 through the two-left-block entry (columns [0, p/2) and [p/2, p) of S passed as separate views)
 * GeneoSetMFMA(0) selects the plain-FMA twin.  reps > 0 also times it (HIP events). */
PetscErrorCode GeneoBlockKernel(int kind, int nsub, const int* suboff, const double* S, int p, const double* T_or_C,
                                int q, double* out, int reps, double* ms_avg);

/* Per-subdomain reductions (dot products of the batched PCG, Z^T x, Gram partials) switch to their cooperative forms --
 * one workgroup per subdomain, once per launch -- above this many 1024-row chunks per subdomain (default 1024, also
 * GENEO_PAR_REDUCE_MIN): the one-subdomain-per-GPU layout of the benchmark's configuration.  Returns the previous value;
 * set it before creating the PC it should govern. */
int GeneoSetParReduceMin(int chunks);
/* fused Rayleigh-Ritz update of one LOBPCG iteration, m = 32 (test hook; host arrays): S, AS, BS n x 96 row-major
 * [X | P | W]; C nsub x 96 x 64; keep / lam / mask nsub x 32.  Out: columns 0..63 of T, AT, BT (n x 96) = [X' P'] of each
 * operand, R (n x 32) = mask .* (A X' - B X' diag(lam)).  AS == NULL: the basis-only form (T from S, C, keep; the other
 * arguments are not touched). */
PetscErrorCode GeneoTestLobpcgUpdate(int nsub, const int* suboff, const double* S, const double* AS, const double* BS,
                                     const double* C, const double* keep, const double* lam, const double* mask,
                                     double* T, double* AT, double* BT, double* R);

/* Test hooks of the backend primitives (csrc/backend.h), one call each, on device pointers of the caller
 * (GeneoDeviceAlloc / GeneoH2D); the argument layout per primitive name is tabulated in tests/primitive_cases.py.
 * Chunked primitives take iarg[0] = nsub and parg[0] = the HOST array suboff (nsub + 1 absolute first rows).
 * Returns the primitive's own result (void: 0, bool: 0 / 1, recip_positive: its count), -1 on an error
 * (PCGenEOGetError(NULL)), -2 for an unknown name. */
int GeneoTestPrimitive(const char* name, const int* iarg, const double* darg, void* const* parg);
/* The same for the primitives of the block entry points (csrc/block_dev.h); argument table in tests/block_rhs_util.py.
 * Returns the primitive's bool as 0 / 1, -1 on an error, -2 for an unknown name. */
int GeneoTestBlockPrimitive(const char* name, const int* iarg, const double* darg, void* const* parg);
/* The same for the Gram-Schmidt primitives of the right-preconditioned GMRES (csrc/krylov_dev.h): vec_gs_dots,
 * vec_gs_update, and vec_gs_group / vec_dot_nwg, which return the group size and the partial sums per vector of a pass;
 * argument table in tests/krylov_right_util.py. */
int GeneoTestKrylovPrimitive(const char* name, const int* iarg, const double* darg, void* const* parg);

/* ---- the coarse operator E on the device at any dimE (-geneo_coarse_device auto|never|always, -geneo_coarse_block nb) ----
 * Where this PC factored E and how it applies E^-1, after the set-up.  factor_on_device: 1 when the blocked device
 * factorisation made the factor, 0 for the host's (Cholesky or LU).  solve_kind: 0 download / host sweeps / upload,
 * 1 the one-workgroup device sweeps (dimE <= 1024), 2 the blocked device sweeps.  block: their block size (0 unless 2). */
PetscErrorCode PCGenEOGetCoarseInfo(PC pc, int* dimE, int* factor_on_device, int* solve_kind, int* block);
/* ---- the Chebyshev local solver (-dls1_ksp_type chebyshev), after the set-up: per local subdomain (in the order they
 * were added) the bounds [lo, hi] used for the V-cycle-preconditioned operator, the degree k_s, and ||b - A x|| / ||b|| of
 * the set-up's verification solve.  Any array may be NULL; at most cap entries are written.  Returns the number of local
 * subdomains, 0 on the cg path, -1 for a bad handle. */
int PCGenEOGetLocalSolverInfo(PC pc, double* lo, double* hi, int* its, double* achieved, int cap);
/* Its coefficient table as the device holds it: coef[(k nsub + s) 2 + {0, 1}] = (a_k, b_k) of local subdomain s, K = max k_s
 * rows, rows k >= k_s of a subdomain exactly zero.  At most cap doubles are written (coef may be NULL); returns K (0 on the
 * cg path), -1 on an error. */
int PCGenEOGetLocalSolverTable(PC pc, double* coef, int cap);
/* What its solves ran since the last set-up: *solves local solves in all, *graph_launches of them replayed from the
 * captured HIP graph (the others went out as direct launches: the first solve, one in eight while the in-situ kernel
 * timer runs, and every solve where capture is unavailable), and *fused_residuals residual updates r - A d taken by the
 * fused sliced kernel (K - 1 per solve when the level-1 matrix is on the sliced path and "cheb_fused" is 1; the others
 * ran the plain product and a vector update).  Any pointer may be NULL.  Returns K (0 on the cg path), -1 for a bad
 * handle. */
int PCGenEOGetLocalSolverCounters(PC pc, long long* solves, long long* graph_launches, long long* fused_residuals);
/* Test hooks of the blocked kernels, HOST arrays (n x n row-major).  GeneoTestCoarseFactor: E = L L^T with block size nb;
 * L lower with a zero strict upper part, LT its transpose, *status 0 or 1 + the index of the first pivot that was not
 * positive.  GeneoTestCoarseSolve: y <- (L L^T)^-1 y, `reps` >= 1 times from the same y (timing).  Every device buffer of
 * the hooks lies between canary pads and is read back: a write outside an array, a changed input or a HIP error is
 * reported.  nb == 0 runs the host code the PC uses without these kernels (host Cholesky; download, host sweeps, upload).
 * GeneoTestCoarseSolveBlock: Y <- (L L^T)^-1 Y on the n x w row-major block Y (w = 16 | 32) by the blocked sweeps on
 * blocks, `reps` >= 1 times from the same Y; Y holds the result of the last one.
 * Returns 0 ok, -1 error (PCGenEOGetError(NULL)), -3 the backend has no such kernels.
 * GeneoTestCoarseElapsed: milliseconds of the last factorisation and of one repetition of the last solve (device time
 * between two events; wall time for nb == 0; -1 before the first call). */
int GeneoTestCoarseFactor(int n, int nb, const double* E, double* L, double* LT, int* status);
int GeneoTestCoarseSolve(int n, int nb, const double* L, const double* LT, double* y, int reps);
int GeneoTestCoarseSolveBlock(int n, int nb, int w, const double* L, const double* LT, double* Y, int reps);
int GeneoTestCoarseElapsed(double* factor_ms, double* solve_ms);
/* cg_start and `iters` steps [spmv, seg_pap, cg_update, cg_direction] of the batched CG on the matrix of `h`
 * (suboff[nsub] rows) with one chunk list alive across the sequence; caller_precond != 0: the form with dinv == NULL in
 * cg_start / cg_update (z = dinv .* r by xmy, seg_partial(r, z, 1), cg_set_rz).  Device vectors; sc_out: host, nsub x 8. */
PetscErrorCode GeneoTestCgSteps(GeneoSpmv h, int nsub, const int* suboff, int iters, double tol2, int caller_precond,
                                const double* b_dev, const double* dinv_dev, double* x_dev, double* r_dev, double* z_dev,
                                double* p_dev, double* sc_out);
/* multigrid set-up operations on CSR (host CSR in and out, device arrays in parg); op 0 csr_remap_columns, 1
 * csr_scaled_alias (+ spmm_fused EPI_PRE), 2 csr_tentative_prolongator (+ spgemm + smooth_prolongator), 3 post_matrix,
 * 4 csr_diag, 5 spgemm + csr_finish + spmv.  Returns nnz of the result (outputs filled when cap >= nnz), -1: product
 * over capacity, -2: error, -3: post_matrix returned false. */
long long GeneoTestCsrOp(int op, const GeneoCsr* A, const GeneoCsr* B, const int* iarg, const double* darg,
                         void* const* parg, int* rowptr_out, int* col_out, double* val_out, long long cap);

/* A stand-alone multigrid hierarchy (test hook; host arrays in, host arrays out, no arithmetic in the hook).
 * Create: A block diagonal with respect to suboff (nsub + 1 first rows, from 0 to A->n), uploaded by the hook and handed
 * to the hierarchy as its resident level-0 matrix.  iparam = {coarse_size, smooth_degree, max_levels, single, max_m,
 * setup, fine_companion}: setup 0 = sparse products on the device, 1 = host set-up + upload; fine_companion != 0 gives the
 * level-0 matrix a single-precision companion of its owner's BEFORE the hierarchy borrows it.  dparam = {smooth_ratio,
 * strength}.  The environment switches of the set-up (GENEO_AMG_*) are read as in a PC.  Returns 0, 1 on an error
 * (PCGenEOGetError(NULL)), 2 when the device set-up declined (a row beyond the product kernels' capacity): nothing is
 * built then and no fallback is taken. */
typedef struct _p_GeneoTestAmg* GeneoTestAmg;
int GeneoTestAmgCreate(const GeneoCsr* A, int nsub, const int* suboff, const int* iparam, const double* dparam,
                       GeneoTestAmg* h);
int GeneoTestAmgDestroy(GeneoTestAmg* h);
int GeneoTestAmgInfo(GeneoTestAmg h, int* nlevels, double* operator_complexity, int* lp_matrices);
/* One level.  iout[11] = {rows, nsub, fused, A.vec_lpr, A.nlong, companions, nnz A, nnz P, nnz R, nnz M, nnz Acs}: nnz -1
 * = the level has no such matrix; companions: bit w set = matrix w (0 A, 1 P, 2 R, 3 M, 4 Acs) carries a
 * single-precision companion.  suboff: nsub + 1, dinv: rows.  Any output may be NULL. */
int GeneoTestAmgLevel(GeneoTestAmg h, int level, long long* iout, double* rho, int* suboff, double* dinv);
/* CSR arrays of matrix `which` (0 A, 1 P, 2 R, 3 M = P - w D^-1 A P, 4 Acs = A diag(dinv)) of a level, as they lie in
 * device memory.  Returns nnz (arrays filled when cap >= nnz; *rows its row count), -1: no such matrix, -2: error. */
long long GeneoTestAmgMatrix(GeneoTestAmg h, int level, int which, int* rows, int* rowptr, int* col, double* val,
                             long long cap);
/* Dense inverses of the coarsest blocks: base[nsub + 1] element offsets, block s row-major at inv + base[s].  Returns
 * base[nsub] (inv filled when cap allows), -2: error. */
long long GeneoTestAmgCoarseInverse(GeneoTestAmg h, long long* base, double* inv, long long cap);
/* X = V_level(B) (AmgDevice::vcycle_from): B rows x ldb, X rows x ldx, m columns used.  Both blocks are uploaded WHOLE,
 * the cycle runs, and both are downloaded whole: padding columns of X and all of B come back as the device left them. */
int GeneoTestAmgVcycle(GeneoTestAmg h, int level, double* B, int ldb, double* X, int ldx, int m);

#ifdef __cplusplus
}
#endif
#endif
