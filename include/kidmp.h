/*
 * kidmp.h -- C ABI of the MI355X-native Thompson-09n column microphysics.
 *
 * This is the drop-in boundary for the one hot path of EnverRamirez/KiD that
 * this project replaces.  Reference files (read-only mount /root/reference):
 *     M: = module_mp_thompson09n.f90        W: = mphys_thompson09n.f90
 * Every entry point names the reference interface it replaces.  Signatures use
 * plain pointers and sizes only; the Fortran side binds them through
 * ISO_C_BINDING (kid_amd/fortran/module_mp_thompson09n.f90).
 *
 * Conventions
 *   - The kidmp_* entries take IEEE binary64 arrays and compute in binary64 (the "P64" build of the
 *     reference: the parity target); the kidmp32_* entries take binary32 arrays (KiD's default REAL).
 *   - A column profile is nz contiguous values, level kts first (k fastest),
 *     i.e. exactly KiD's `theta(k,i)` storage (W:60-93).  A batch of ncol
 *     columns is x[col*nz + k].
 *   - Every function returns 0 on success or a negative KIDMP_E* code; it
 *     never aborts and never throws.  kidmp_last_error() gives the text.
 *   - Every entry point makes the context's device current for the duration of the call and restores the
 *     caller's; device pointers must belong to the context's device (KIDMP_EINVAL otherwise).
 *   - One context per process and device; calls on one context are
 *     serialised by the caller (the reference is single-threaded, M:386-430),
 *     and its asynchronous launches must not overlap on the device (enqueue
 *     them on one stream): a context owns one work buffer.
 */
#ifndef KIDMP_H
#define KIDMP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KIDMP_OK            0
#define KIDMP_EINVAL       -1   /* bad argument (null pointer, nz out of range ...) */
#define KIDMP_ENODEV       -2   /* no HIP device / wrong architecture            */
#define KIDMP_EHIP         -3   /* a HIP runtime call failed                      */
#define KIDMP_ENOMEM       -4
#define KIDMP_ESTATE       -5   /* context not initialised / already finalised    */
#define KIDMP_EIO          -6   /* cache file missing, unreadable or malformed    */

#define KIDMP_MAX_NZ      256   /* levels per column supported by the kernels     */
#define KIDMP_NRATES       36   /* process-rate diagnostics, order of M:2967-3119 */

typedef struct kidmp_ctx kidmp_ctx;

/* Run-time switches the reference reads from KiD modules:
 *   iiwarm, set_Nc      `namelists` (M:22)
 *   l_sediment          `switches`  (M:20)  gates ice/snow/graupel fall only
 *   device              HIP device ordinal (one process per GPU)
 *   is_aerosol_aware    `module_mp_thompson09n`'s public LOGICAL (M:28)          */
typedef struct kidmp_cfg {
    int32_t iiwarm;
    int32_t l_sediment;
    double  set_Nc;        /* cloud droplet number, cm^-3 (Nt_c = set_Nc*1e6, M:381) */
    int32_t device;
    int32_t is_aerosol_aware;   /* the module's public switch (M:28; .false. in KiD): prognostic droplet number, aerosol
                                   activation / DeMott / Koop nucleation, scavenging, droplet evaporation */
} kidmp_cfg;

/* thompson_init (M:374-797): computes the gamma/rate constants on the host and
 * builds the lookup tables (M:3698-4343) with HIP kernels into HBM. */
int kidmp_init(const kidmp_cfg *cfg, kidmp_ctx **ctx_out);
void kidmp_finalize(kidmp_ctx *ctx);
const char *kidmp_last_error(const kidmp_ctx *ctx);

/* mp_thompson (M:1156-3688), host arrays, one column: the compatibility entry
 * behind the Fortran `mp_thompson` shim.  The 12 profiles are INOUT, p1d/w1d/
 * dzq IN, ppt[4] = {pptrain, pptsnow, pptgraul, pptice} INOUT (accumulated),
 * as in the reference dummy list (M:1156-1177). */
int kidmp_column_step(kidmp_ctx *ctx, int32_t nz, double dt,
                      double *qv1d, double *qc1d, double *qi1d, double *qr1d,
                      double *qs1d, double *qg1d, double *ni1d, double *nr1d,
                      double *nc1d, double *nwfa1d, double *nifa1d, double *t1d,
                      const double *p1d, const double *w1d, const double *dzq,
                      double *ppt);

/* The `do i=1,nx` loop of the KiD adapter (W:54-246) as ONE batched call on
 * host arrays x[col*nz+k]; ppt is [ncol][4] (INOUT).  rates may be NULL, else
 * receives [ncol][KIDMP_NRATES][nz] (the save_dg values of M:2962-3124).
 * Arrays KiD itself never fills may be left out (NULL) in all three host-array entries; they then neither cross
 * PCIe nor come back:
 *   nc, nwfa, nifa (all three or none)   contexts without is_aerosol_aware: the adapter passes them unset (W:36);
 *                                        the non-aerosol defaults of M:958-964 are formed on the device
 *   qi, qs, qg, ni (all four or none)    iiwarm contexts: a warm run keeps the frozen species at zero (W:46-52)
 *   w                                    contexts without is_aerosol_aware (never read)
 * A context that reads them (aerosol-aware / mixed-phase) refuses the call instead. */
int kidmp_batch_step_host(kidmp_ctx *ctx, int64_t ncol, int32_t nz, double dt,
                          double *qv, double *qc, double *qi, double *qr,
                          double *qs, double *qg, double *ni, double *nr,
                          double *nc, double *nwfa, double *nifa, double *t,
                          const double *p, const double *w, const double *dz,
                          double *ppt, double *rates);

/* Same, also returning the substep counts: nstep (may be NULL) receives [ncol][4] int32 (rain, ice, snow,
 * graupel; M:3365,3447,3504,3553).  All four are 0 for a column that left through the `no_micro` early return
 * (M:1540) -- such a column makes no save_dg call in the reference, which is how the Fortran drop-in knows to
 * skip it when it replays the rate diagnostics. */
int kidmp_batch_step_host_diag(kidmp_ctx *ctx, int64_t ncol, int32_t nz, double dt,
                               double *qv, double *qc, double *qi, double *qr,
                               double *qs, double *qg, double *ni, double *nr,
                               double *nc, double *nwfa, double *nifa, double *t,
                               const double *p, const double *w, const double *dz,
                               double *ppt, double *rates, int32_t *nstep);

/* Same, on DEVICE pointers (state resident in HBM), enqueued on `stream`
 * (a hipStream_t passed as void*; NULL = the null stream).  Asynchronous.
 * nstep (may be NULL) receives [ncol][4] int32 substep counts (rain, ice,
 * snow, graupel; M:3365,3447,3504,3553). */
int kidmp_batch_step_device(kidmp_ctx *ctx, int64_t ncol, int32_t nz, double dt,
                            double *qv, double *qc, double *qi, double *qr,
                            double *qs, double *qg, double *ni, double *nr,
                            double *nc, double *nwfa, double *nifa, double *t,
                            const double *p, const double *w, const double *dz,
                            double *ppt, double *rates, int32_t *nstep,
                            void *stream);

/* ---- The same three entries on binary32 arrays: the reference's `REAL` when KiD is built with its default
 * 4-byte reals (M:1168-1177 declares every dummy REAL).  `arith` selects the arithmetic inside the kernel:
 *   KIDMP_ARITH_P32N  the reference as shipped: everything it declares REAL is binary32, everything it declares
 *                     DOUBLE PRECISION (the ~70 process rates M:1184-1211, ilamr/ilamg/N0_r/N0_g M:1225, lamc/lamr/
 *                     lamg/lami/N0_exp M:1235-1236, the lookup tables) stays binary64;
 *   KIDMP_ARITH_F32   everything binary32 (the cheap end of the precision sweep of BASELINE config 5).
 * rates (may be NULL) is binary64 in both.  The double entries above are the parity build (P64). */
#define KIDMP_ARITH_P32N 0
#define KIDMP_ARITH_F32  1
int kidmp32_column_step(kidmp_ctx *ctx, int32_t nz, float dt,
                        float *qv1d, float *qc1d, float *qi1d, float *qr1d,
                        float *qs1d, float *qg1d, float *ni1d, float *nr1d,
                        float *nc1d, float *nwfa1d, float *nifa1d, float *t1d,
                        const float *p1d, const float *w1d, const float *dzq,
                        float *ppt, int32_t arith);
int kidmp32_batch_step_host(kidmp_ctx *ctx, int64_t ncol, int32_t nz, float dt,
                            float *qv, float *qc, float *qi, float *qr,
                            float *qs, float *qg, float *ni, float *nr,
                            float *nc, float *nwfa, float *nifa, float *t,
                            const float *p, const float *w, const float *dz,
                            float *ppt, double *rates, int32_t *nstep, int32_t arith);
int kidmp32_batch_step_device(kidmp_ctx *ctx, int64_t ncol, int32_t nz, float dt,
                              float *qv, float *qc, float *qi, float *qr,
                              float *qs, float *qg, float *ni, float *nr,
                              float *nc, float *nwfa, float *nifa, float *t,
                              const float *p, const float *w, const float *dz,
                              float *ppt, double *rates, int32_t *nstep,
                              int32_t arith, void *stream);

/* DEPRECATED, kept for hosts linked against earlier builds: rounds 1-2 reserved a per-batch work profile here.  The step
 * owns no per-batch device memory any more; the call checks its arguments, does nothing and returns KIDMP_OK. */
int kidmp_reserve(kidmp_ctx *ctx, int64_t ncol, int32_t nz);

/* The device entries own no per-batch device memory and never allocate: they can be captured into a hipGraph as
 * they are, and one context may have STEP launches in flight on several streams.  (The diagnostics entries further
 * down -- kidmp_reduce_rates_device, kidmp_sanity_device -- use one scratch buffer per context, allocated by
 * kidmp_init: they never allocate either, but calls of one of them on ONE context must be enqueued on one stream.) */

/* ---- host memory for the host-array entries (kidmp_batch_step_host*, kidmp32_batch_step_host) ----
 * Those entries stand where the reference's `do i=1,nx` loop works on the model's own arrays (W:54-246), so every
 * call moves the state across PCIe: 14 profiles in, 12 out per column (about 25 KB in binary64).  They run as a
 * three-stage pipeline over column chunks -- upload of chunk i+1, step of chunk i, download of chunk i-1 on three
 * streams -- which only overlaps if the DMA engines can reach the host arrays, i.e. if they are page-locked.
 * kidmp_host_alloc returns page-locked memory (NULL on failure, message in kidmp_last_error(NULL)); free it with
 * kidmp_host_free (memory the caller got from hipHostMalloc serves as well; for hipHostRegister see INTEGRATION.md 4).  Pageable
 * arrays are accepted too: results are the same, the copies are then staged by the HIP runtime and do not overlap.
 * Neither function needs a context. */
void *kidmp_host_alloc(size_t bytes);
void kidmp_host_free(void *p);
/* Columns per pipeline chunk of this context's host-array entries; 0 (default) = a quarter of the batch, rounded up
 * to 256, at most 8 192 (one chunk for batches of <= 2048 columns). */
int kidmp_set_host_chunk(kidmp_ctx *ctx, int64_t ncol_per_chunk);

/* Non-aerosol defaults for nc1d/nwfa1d/nifa1d, which the KiD wrapper leaves
 * unset (W:36): nc=Nt_c/rho, nwfa=11.1e6/rho, nifa=naIN1*0.01/rho with
 * rho=0.622p/(R T (qv+0.622)) (M:958-964).  Device pointers, [ncol*nz]. */
int kidmp_default_aerosols_device(kidmp_ctx *ctx, int64_t n,
                                  const double *qv, const double *t, const double *p,
                                  double *nc, double *nwfa, double *nifa, void *stream);

/* Domain sums of the surface precipitation (the analogue of the nx-means of
 * W:248-275): out[4] (device pointer) = sum over columns of ppt[col][0..3].
 * Multi-GPU callers all-reduce out[4] with RCCL afterwards. */
int kidmp_reduce_ppt_device(kidmp_ctx *ctx, int64_t ncol, const double *ppt,
                            double *out4, void *stream);

/* The same four sums EXACTLY, whatever the order of the additions and however the columns are spread over devices:
 * limbs (device, int64[KIDMP_PPT_LIMBS]) receives fixed-point accumulators (per species 6 limbs, limb j weighs
 * 2**(32j-128); values below 2**-128 are dropped, |x| must stay below 2**32).  Integer sums are associative, so
 * multi-GPU callers all-reduce(SUM, int64) the limbs and every partition of the columns yields the same bits;
 * kidmp_ppt_limbs_to_sums turns (host) limbs into the four doubles. */
#define KIDMP_PPT_LIMBS 24
int kidmp_reduce_ppt_exact_device(kidmp_ctx *ctx, int64_t ncol, const double *ppt, int64_t *limbs, void *stream);
int kidmp_ppt_limbs_to_sums(const int64_t *limbs, double *out4);

/* ---- several GPUs behind one call: the `do i=1,nx` loop of the KiD adapter (W:54-246) over a device list ----
 * The reference's compiled-out decomposition (M:3744-3746, M:3813-3819) splits work over MPI ranks; KiD itself is one
 * process.  kidmp_init_multi builds one context per entry of devices[] (thompson_init on every device, tables built per
 * device); kidmp_batch_step_host_multi cuts the ncol host columns into contiguous ranges (kidmp_shard_bounds: sizes
 * differ by at most one, range i on devices[i]), runs every range through its context's own upload / step / download
 * pipeline concurrently (one host thread per context), and returns in precip_sums[4] (may be NULL) the domain sums of
 * ppt -- the numerators of the nx-means of W:248-303 -- reduced over the devices with ONE RCCL all-reduce (int64 SUM of
 * the exact accumulators above; librccl.so is dlopen'ed by kidmp_init_multi, a one-GPU host never needs it).  No halo,
 * no other exchange.  Results per column are those of kidmp_batch_step_host_diag bit for bit, the sums are identical
 * for every device list.  A device may be named twice (two contexts on one card).  Optional arrays as above. */
typedef struct kidmp_multi kidmp_multi;
#define KIDMP_MAX_DEVICE_LIST 16     /* entries of devices[]; a process may hold 32 contexts at once */
int kidmp_init_multi(const kidmp_cfg *cfg, int32_t ndev, const int32_t *devices, kidmp_multi **out);   /* cfg->device is ignored */
void kidmp_finalize_multi(kidmp_multi *m);
const char *kidmp_multi_last_error(const kidmp_multi *m);
int32_t kidmp_multi_size(const kidmp_multi *m);
kidmp_ctx *kidmp_multi_context(kidmp_multi *m, int32_t i);         /* e.g. for kidmp_load_table_cache on every device */
int kidmp_shard_bounds(int64_t ncol, int32_t nshard, int32_t shard, int64_t *lo, int64_t *hi);   /* no GPU needed */
int kidmp_batch_step_host_multi(kidmp_multi *m, int64_t ncol, int32_t nz, double dt,
                                double *qv, double *qc, double *qi, double *qr,
                                double *qs, double *qg, double *ni, double *nr,
                                double *nc, double *nwfa, double *nifa, double *t,
                                const double *p, const double *w, const double *dz,
                                double *ppt, double *rates, int32_t *nstep, double *precip_sums);
/* The same call with the sanity scan of the scheme's 3-D driver (M:1025-1094) over the END state of all ncol columns:
 * sanity15 (host, may be NULL) = what kidmp_sanity_device returns for the unsharded batch -- [0..6] maxima of qc, qr, nr,
 * qs, qi, qg, ni, [7..14] numbers of negative entries of qc, qr, nr, qs, qi, qg, ni, qv --, scanned chunk by chunk on each
 * device as the chunks leave the step (exact integer atomics) and reduced over the devices beside the precipitation
 * limbs, in the same RCCL group: all-reduce(uint64, MAX) of the seven maxima (non-negative doubles order like their bit
 * patterns), all-reduce(uint64, SUM) of the eight counts.  Identical for every device list. */
int kidmp_batch_step_host_multi_diag(kidmp_multi *m, int64_t ncol, int32_t nz, double dt,
                                     double *qv, double *qc, double *qi, double *qr,
                                     double *qs, double *qg, double *ni, double *nr,
                                     double *nc, double *nwfa, double *nifa, double *t,
                                     const double *p, const double *w, const double *dz,
                                     double *ppt, double *rates, int32_t *nstep, double *precip_sums, double *sanity15);

/* Optional domain diagnostics beyond the four precipitation sums.
 * kidmp_reduce_rates_device: out[KIDMP_NRATES*nz] (device) = sum over columns of rates[col][r][k] -- the mean
 *   process-rate profiles KiD plots are these sums / ncol (save_dg(k, value, ...) of M:2967-3119, averaged over nx);
 *   fixed summation order, so the result is reproducible.  Multi-GPU callers all-reduce(SUM) it.
 * kidmp_sanity_device: the scan the scheme's own 3-D driver runs after each column (M:1025-1094):
 *   out15[0..6] = max over all n = ncol*nz entries of qc, qr, nr, qs, qi, qg, ni; out15[7..14] = how many entries of
 *   qc, qr, nr, qs, qi, qg, ni, qv are negative (the reference formats a WARNING for each).  Multi-GPU callers
 *   all-reduce(MAX) the first seven and all-reduce(SUM) the rest.
 * Both use per-context scratch from kidmp_init (see above): per context, enqueue them on one stream. */
int kidmp_reduce_rates_device(kidmp_ctx *ctx, int64_t ncol, int32_t nz, const double *rates, double *out, void *stream);
int kidmp_sanity_device(kidmp_ctx *ctx, int64_t n, const double *qc, const double *qr, const double *nr,
                        const double *qs, const double *qi, const double *qg, const double *ni, const double *qv,
                        double *out15, void *stream);

/* calc_effectRad (M:4834-4935): radiation effective radii of cloud water, cloud ice and snow, consistent with the
 * scheme's size distributions.  n = ncol*nz elements (every level stands alone); re_qc/re_qi/re_qs are INOUT like the
 * reference's (a level without the species keeps the caller's value, M:4873 / 4888 / 4897; the scheme's 3-D driver
 * presets 2.49E-6, 4.99E-6, 9.99E-6 m and clamps afterwards, M:1111-1121).
 *   kidmp_effective_radii_device    device pointers, asynchronous on `stream`; every array required
 *   kidmp_effective_radii_host      host arrays (the compatibility procedure behind the Fortran calc_effectRad), moved in
 *                                   chunks of kidmp_set_host_chunk columns of a nominal 128 levels
 *   kidmp32_effective_radii_device, kidmp32_effective_radii_host   binary32 arrays: inputs widened to binary64, the same
 *                                   binary64 arithmetic, the result rounded to binary32 once (not the reference's native
 *                                   binary32 arithmetic)
 * The host entry and the kidmp32_* entries accept what a caller may not have: nc NULL in a context that is not
 * aerosol-aware (nc = Nt_c there, M:4863; an aerosol-aware context needs it), and in an iiwarm context qi + ni NULL, qs
 * NULL (zero) and re_qi + re_qs NULL (not formed). */
int kidmp_effective_radii_device(kidmp_ctx *ctx, int64_t n, const double *t, const double *p, const double *qv,
                                 const double *qc, const double *nc, const double *qi, const double *ni,
                                 const double *qs, double *re_qc, double *re_qi, double *re_qs, void *stream);
int kidmp_effective_radii_host(kidmp_ctx *ctx, int64_t n, const double *t, const double *p, const double *qv,
                               const double *qc, const double *nc, const double *qi, const double *ni,
                               const double *qs, double *re_qc, double *re_qi, double *re_qs);
int kidmp32_effective_radii_device(kidmp_ctx *ctx, int64_t n, const float *t, const float *p, const float *qv,
                                   const float *qc, const float *nc, const float *qi, const float *ni,
                                   const float *qs, float *re_qc, float *re_qi, float *re_qs, void *stream);
int kidmp32_effective_radii_host(kidmp_ctx *ctx, int64_t n, const float *t, const float *p, const float *qv,
                                 const float *qc, const float *nc, const float *qi, const float *ni,
                                 const float *qs, float *re_qc, float *re_qi, float *re_qs);

/* calc_refl10cm (M:4946-5244): 10-cm radar reflectivity (Rayleigh, dBZ) of rain, snow and graupel from the scheme's own
 * size distributions -- what WRF and MPAS write as REFL_10CM.  Every level of every column receives
 * dbz = 10*log10((ze_rain + ze_snow + ze_graupel)*1e18) (M:5196); a level without precipitation gets 10*log10(3e-4).
 * Reproduces the reference as shipped: no bright band (its wet-snow / wet-graupel branch is dead with nrbins = 0, M:204).
 * The graupel intercept is a top-down running minimum over the column, so whole columns are needed: arrays are
 * x[col*nz + k] as everywhere in this header, k = 0 the lowest level (kts).  qc1d is never read by the reference and is
 * not taken.  qs and qg may both be NULL in an iiwarm context (zero).  IN: t, p, qv, qr, nr, qs, qg; OUT: dbz.
 *   kidmp_reflectivity_device     device pointers, asynchronous on `stream`; no allocation
 *   kidmp_reflectivity_host       host arrays (the compatibility procedure behind the Fortran calc_refl10cm)
 * The kidmp32_* forms take binary32 arrays: inputs widened to binary64, the same binary64 arithmetic as the kidmp_*
 * forms, the result rounded to binary32 once (not the reference's native binary32 arithmetic). */
int kidmp_reflectivity_device(kidmp_ctx *ctx, int64_t ncol, int32_t nz, const double *t, const double *p,
                              const double *qv, const double *qr, const double *nr, const double *qs, const double *qg,
                              double *dbz, void *stream);
int kidmp32_reflectivity_device(kidmp_ctx *ctx, int64_t ncol, int32_t nz, const float *t, const float *p,
                                const float *qv, const float *qr, const float *nr, const float *qs, const float *qg,
                                float *dbz, void *stream);
int kidmp_reflectivity_host(kidmp_ctx *ctx, int64_t ncol, int32_t nz, const double *t, const double *p,
                            const double *qv, const double *qr, const double *nr, const double *qs, const double *qg,
                            double *dbz);
int kidmp32_reflectivity_host(kidmp_ctx *ctx, int64_t ncol, int32_t nz, const float *t, const float *p,
                              const float *qv, const float *qr, const float *nr, const float *qs, const float *qg,
                              float *dbz);
/* kidmp_batch_step_host_diag / kidmp32_batch_step_host followed, chunk by chunk on the device, by the reflectivity of the
 * post-step state: dbz (host, [ncol][nz]) is the only extra array that crosses PCIe.  dbz NULL = the plain entry.
 * State, ppt, rates and nstep are those of the plain entry bit for bit. */
int kidmp_batch_step_host_refl(kidmp_ctx *ctx, int64_t ncol, int32_t nz, double dt,
                               double *qv, double *qc, double *qi, double *qr,
                               double *qs, double *qg, double *ni, double *nr,
                               double *nc, double *nwfa, double *nifa, double *t,
                               const double *p, const double *w, const double *dz,
                               double *ppt, double *rates, int32_t *nstep, double *dbz);
int kidmp32_batch_step_host_refl(kidmp_ctx *ctx, int64_t ncol, int32_t nz, float dt,
                                 float *qv, float *qc, float *qi, float *qr,
                                 float *qs, float *qg, float *ni, float *nr,
                                 float *nc, float *nwfa, float *nifa, float *t,
                                 const float *p, const float *w, const float *dz,
                                 float *ppt, double *rates, int32_t *nstep, int32_t arith, float *dbz);

/* ---- the column outputs: what a host model takes from the state beside the step ----
 * The scheme's own driver forms the effective radii from each column right after the step (M:1109-1121: presets, then
 * calc_effectRad, M:4834-4935), and WRF / MPAS form REFL_10CM (calc_refl10cm, M:4946-5244) beside them.  These entries
 * return any of the four profiles; when the radii AND dbz are wanted, one kernel forms them from a single read of the
 * column (one wavefront per column).
 *   dbz                    may be NULL; as kidmp_reflectivity_*
 *   re_qc, re_qi, re_qs    requested together or not at all; in an iiwarm context re_qi and re_qs may be NULL beside
 *                          re_qc.  OUT, in the driver's form: a level without the species receives the preset 2.49E-6 /
 *                          4.99E-6 / 9.99E-6 m (M:1111-1113); the driver's clamps after the call (M:1118-1120) change nothing
 *                          after the subroutine's own.  Values are those of kidmp_effective_radii_* started from the presets.
 * Nothing requested (out NULL or all four NULL) = the plain call.  kidmp32_*: binary32 arrays, binary64 arithmetic, one
 * rounding, as above. */
typedef struct kidmp_outputs   { double *dbz, *re_qc, *re_qi, *re_qs; } kidmp_outputs;
typedef struct kidmp32_outputs { float  *dbz, *re_qc, *re_qi, *re_qs; } kidmp32_outputs;
/* Device pointers [ncol*nz], asynchronous on `stream`, no allocation: capturable into a hipGraph like the step.
 * IN: t, p, qv; qc, nc, qi, ni (radii); qr, nr (dbz); qs, qg (both).  nc may be NULL unless the context is aerosol-aware;
 * qi + ni and qs + qg may be NULL pairwise in an iiwarm context (zero). */
int kidmp_column_outputs_device(kidmp_ctx *ctx, int64_t ncol, int32_t nz, const double *t, const double *p,
                                const double *qv, const double *qc, const double *nc, const double *qi, const double *ni,
                                const double *qr, const double *nr, const double *qs, const double *qg,
                                const kidmp_outputs *out, void *stream);
int kidmp32_column_outputs_device(kidmp_ctx *ctx, int64_t ncol, int32_t nz, const float *t, const float *p,
                                  const float *qv, const float *qc, const float *nc, const float *qi, const float *ni,
                                  const float *qr, const float *nr, const float *qs, const float *qg,
                                  const kidmp32_outputs *out, void *stream);
/* kidmp_batch_step_host_diag / kidmp32_batch_step_host followed, chunk by chunk on the device, by ONE launch that forms the
 * requested outputs (host arrays [ncol][nz]) from the chunk's post-step state; only requested profiles are staged and
 * cross PCIe.  State, ppt, rates and nstep are those of the plain entry bit for bit; kidmp[32]_batch_step_host_refl are
 * this call with dbz alone. */
int kidmp_batch_step_host_out(kidmp_ctx *ctx, int64_t ncol, int32_t nz, double dt,
                              double *qv, double *qc, double *qi, double *qr,
                              double *qs, double *qg, double *ni, double *nr,
                              double *nc, double *nwfa, double *nifa, double *t,
                              const double *p, const double *w, const double *dz,
                              double *ppt, double *rates, int32_t *nstep, const kidmp_outputs *out);
int kidmp32_batch_step_host_out(kidmp_ctx *ctx, int64_t ncol, int32_t nz, float dt,
                                float *qv, float *qc, float *qi, float *qr,
                                float *qs, float *qg, float *ni, float *nr,
                                float *nc, float *nwfa, float *nifa, float *t,
                                const float *p, const float *w, const float *dz,
                                float *ppt, double *rates, int32_t *nstep, int32_t arith, const kidmp32_outputs *out);

/* ---- a droplet number per column: Nd ensembles in one launch ----
 * set_Nc (KiD namelists, M:22) enters the scheme only as Nt_c = set_Nc*1.e6 (M:381): no lookup table depends on it and
 * nu_c is formed per level, so one context and one set of tables serve any mix of values.  kidmp_set_column_nc binds an
 * array of ncol values to the context; while it is bound, column c of every batch uses Nt_c = set_nc[c]*1.e6 wherever the
 * context's scalar is read on the device: the column step (M:1410, M:2081, M:2602, M:2799), calc_effectRad (M:4863) and
 * the default aerosols (nc = Nt_c/rho, M:960).  A uniform array reproduces a context initialised with that value bit for
 * bit; without a binding every entry returns the bits it returned before.  calc_refl10cm does not read Nt_c.
 *   IN   set_nc   [ncol] binary64 (also for the kidmp32_* entries), cm**-3, host or device memory.  Copied into a buffer
 *                 the context owns: the call allocates, is synchronous, and the caller's array may be freed afterwards.
 *                 The step entries still never allocate and stay capturable into a hipGraph.
 *                 ncol == 0 or set_nc NULL unbinds.  kidmp_column_nc_count: the bound count, 0 when nothing is bound.
 *   refused (KIDMP_EINVAL, the previous binding stays): a value that is not finite and > 0 -- what kidmp_init demands of
 *                 cfg->set_Nc; the message names the first such column -- and an aerosol-aware context (n_c is prognostic).
 * While a binding is active (KIDMP_EINVAL otherwise, no array touched):
 *   kidmp[32]_column_step (count 1), kidmp[32]_batch_step_device, kidmp[32]_batch_step_host / _diag / _refl / _out and
 *   kidmp[32]_column_outputs_device take ncol == the bound count; the host pipeline offsets into the bound buffer by each
 *   chunk's first column, so nothing extra crosses PCIe per call;
 *   kidmp[32]_effective_radii_{device,host} and kidmp_default_aerosols_device, which have n and no nz, take n as a
 *   multiple of the bound count: nz = n / count, element e belongs to column e / nz;
 *   kidmp_batch_step_host_multi[_diag] refuse a multi handle one of whose member contexts holds a binding: sharding the
 *   array over devices is not implemented.
 * kidmp_get_const("Nt_c") keeps returning the context's scalar. */
int kidmp_set_column_nc(kidmp_ctx *ctx, int64_t ncol, const double *set_nc);
int64_t kidmp_column_nc_count(const kidmp_ctx *ctx);

/* ---- mphys_thompson09_interfacen (W:28-310): the KiD adapter, theta-form state in, tendencies out ----
 * One call takes KiD's own fields and returns the microphysics tendencies and the surface precipitation:
 *   gather (W:46-97, one launch)   t = (theta + (dtheta_adv + dtheta_div)*dt)*exner, X1 = X + (dX_adv + dX_div)*dt for
 *                                  q_v and the hydrometeor moments, p = p0*exner**(1./r_on_cp) (formed on the device),
 *                                  dz broadcast from KiD's one profile, w = 0, the frozen species exact zeros in an iiwarm
 *                                  context (W:46-52), nc / nwfa / nifa the non-aerosol defaults of M:958-964 (the bits of
 *                                  kidmp_default_aerosols_device on the gathered t, qv, p), ppt zeroed (W:55-58)
 *   mp_thompson                    the column step of kidmp_batch_step_device on the gathered state
 *   the column outputs             `out` as in kidmp_column_outputs_device, of the post-step state
 *   back-out (W:198-245, one launch)   dtheta_mphys = (t/exner - theta)/dt - (dtheta_adv + dtheta_div),
 *                                  dX_mphys = (X1 - X)/dt - (dX_adv + dX_div); /dt is a division
 * Every operation is rounded in the arrays' format.  Fields are [ncol][nz] (KiD's theta(k,i) storage, W:60-93), dz is
 * ONE profile of nz values, ppt is [ncol][4] = {rain, snow, graupel, ice}.
 *   state   IN, never written.  theta, qv, qc, qr, nr always; qi, ni, qs, qg in a mixed-phase context.
 *   adv, div   the advective and divergence tendencies.  Each may be NULL as a whole and any member may be NULL: NULL
 *           means zero (never read; the results are bit for bit those of an array of +0.0).
 *   mphys   OUT: the tendencies, same members as `state` (theta = dtheta_mphys, qv = dqv_mphys, the seven moments =
 *           dhydrometeors_mphys).  A mixed-phase context requires the frozen members of `state` and `mphys`.
 *   In an iiwarm context the frozen members (qi, ni, qs, qg) of state, adv, div and mphys are neither read nor written
 *   and may be NULL.
 *   ppt     OUT, not INOUT (W:55-58).  rates, nstep, out: optional, as for the step and the column outputs.
 *   Output arrays must not overlap any input array (stated, not checked).
 *   work    the device entries' workspace of kidmp_kid_workspace_bytes(ncol, nz) bytes, 16-byte aligned: 15 profiles of
 *           ncol*nz values, each stride rounded up to 256 bytes; profile v starts at kidmp_kid_workspace_offset(ncol, nz, v):
 *           0..11 = qv, qc, qi, qr, qs, qg, ni, nr, nc, nwfa, nifa, t (the order of mp_thompson's dummies, M:1156), 12 = p,
 *           13 = w, 14 = dz.  After the call it holds the post-step T/q state: `out` is formed from it.
 * The device entries never allocate, enqueue only on `stream` (gather, step, outputs, back-out: one linear chain) and
 * can be captured into a hipGraph.  A bound per-column droplet number (kidmp_set_column_nc) is honoured; ncol must equal
 * the bound count, as for the step.  The host entries run chunk by chunk inside the three-stream pipeline of
 * kidmp_batch_step_host (upload of the present members of state, adv, div and exner; dz once; download of mphys, ppt and
 * what else was requested); results are those of the device entry bit for bit for any chunking (kidmp_set_host_chunk).
 * Refused with KIDMP_EINVAL, nothing written: a workspace that is too small, a missing required pointer, nz outside
 * [2, KIDMP_MAX_NZ], dt <= 0, a pointer of another device.  A NULL context returns KIDMP_ESTATE; ncol == 0 KIDMP_OK.
 * kidmp_kid_workspace_bytes / _offset need no context and no GPU and return 0 for bad arguments (ncol < 0, nz outside
 * [1, KIDMP_MAX_NZ], v outside [0, 14]).  The kidmp32_* forms take binary32 arrays and `arith` like the step; p is then
 * pow(double(exner), double(1.f/r_on_cp)) rounded once to binary32 (a correctly rounded powf), times p0 in binary32. */
typedef struct kidmp_kid_fields   { double *theta, *qv, *qc, *qr, *nr, *qi, *ni, *qs, *qg; } kidmp_kid_fields;    /* each [ncol][nz] */
typedef struct kidmp32_kid_fields { float  *theta, *qv, *qc, *qr, *nr, *qi, *ni, *qs, *qg; } kidmp32_kid_fields;
size_t kidmp_kid_workspace_bytes(int64_t ncol, int32_t nz);
size_t kidmp_kid_workspace_offset(int64_t ncol, int32_t nz, int32_t v);
size_t kidmp32_kid_workspace_bytes(int64_t ncol, int32_t nz);
size_t kidmp32_kid_workspace_offset(int64_t ncol, int32_t nz, int32_t v);
int kidmp_kid_interface_device(kidmp_ctx *ctx, int64_t ncol, int32_t nz, double dt, double p0, double r_on_cp,
                               const kidmp_kid_fields *state, const kidmp_kid_fields *adv, const kidmp_kid_fields *div,
                               const double *exner, const double *dz, const kidmp_kid_fields *mphys, double *ppt,
                               double *rates, int32_t *nstep, const kidmp_outputs *out,
                               void *work, size_t work_bytes, void *stream);
int kidmp_kid_interface_host(kidmp_ctx *ctx, int64_t ncol, int32_t nz, double dt, double p0, double r_on_cp,
                             const kidmp_kid_fields *state, const kidmp_kid_fields *adv, const kidmp_kid_fields *div,
                             const double *exner, const double *dz, const kidmp_kid_fields *mphys, double *ppt,
                             double *rates, int32_t *nstep, const kidmp_outputs *out);
int kidmp32_kid_interface_device(kidmp_ctx *ctx, int64_t ncol, int32_t nz, float dt, float p0, float r_on_cp,
                                 const kidmp32_kid_fields *state, const kidmp32_kid_fields *adv, const kidmp32_kid_fields *div,
                                 const float *exner, const float *dz, const kidmp32_kid_fields *mphys, float *ppt,
                                 double *rates, int32_t *nstep, const kidmp32_outputs *out, int32_t arith,
                                 void *work, size_t work_bytes, void *stream);
int kidmp32_kid_interface_host(kidmp_ctx *ctx, int64_t ncol, int32_t nz, float dt, float p0, float r_on_cp,
                               const kidmp32_kid_fields *state, const kidmp32_kid_fields *adv, const kidmp32_kid_fields *div,
                               const float *exner, const float *dz, const kidmp32_kid_fields *mphys, float *ppt,
                               double *rates, int32_t *nstep, const kidmp32_outputs *out, int32_t arith);
/* The gather alone: fills the workspace with the step's inputs (the pre-step state, p, w, dz, the default aerosols) and
 * zeroes ppt, for a host that runs kidmp[32]_batch_step_device on the workspace itself, and for the tests.  Arguments,
 * checks and refusals as above. */
int kidmp_kid_gather_device(kidmp_ctx *ctx, int64_t ncol, int32_t nz, double dt, double p0, double r_on_cp,
                            const kidmp_kid_fields *state, const kidmp_kid_fields *adv, const kidmp_kid_fields *div,
                            const double *exner, const double *dz, double *ppt, void *work, size_t work_bytes, void *stream);
int kidmp32_kid_gather_device(kidmp_ctx *ctx, int64_t ncol, int32_t nz, float dt, float p0, float r_on_cp,
                              const kidmp32_kid_fields *state, const kidmp32_kid_fields *adv, const kidmp32_kid_fields *div,
                              const float *exner, const float *dz, float *ppt, void *work, size_t work_bytes, void *stream);

/* Introspection for parity tests: copy a lookup table / constant array to the
 * host.  Names are the reference's (tcg_racg ... t_Efsw; cre, crg, Dr ...).
 * Returns the number of doubles (<0 on error); out may be NULL to query. */
int64_t kidmp_get_table(kidmp_ctx *ctx, const char *name, double *out, int64_t cap);
int64_t kidmp_get_const(kidmp_ctx *ctx, const char *name, double *out, int64_t cap);

/* Interop with the reference's table cache (the only checkpoint-like facility of the path, M:3717-3829 and
 * M:3864-4078): list-directed text files run_data/racg_thompson09.data (6 tables) and
 * run_data/racs_thompson09.data (12 tables).  kidmp_save_table_cache writes the GPU-built tables so that a
 * stock KiD run with l_reuse_thompson_lookup=.true. can read them; kidmp_load_table_cache replaces this
 * context's rain-graupel / rain-snow tables by the files' contents (e.g. written by the reference).
 * `dir` is the directory holding the two files (the reference hard-codes "run_data"). */
int kidmp_save_table_cache(kidmp_ctx *ctx, const char *dir);
int kidmp_load_table_cache(kidmp_ctx *ctx, const char *dir);
/* thompson_init's own use of the two files, as the reference does it per file (M:3717-3729 / M:3822-3829 for racg,
 * M:3864-3895 / M:4065-4078 for racs): if the file exists AND l_reuse (KiD's switch l_reuse_thompson_lookup, M:20) its
 * tables replace the GPU-built ones; otherwise the GPU-built tables are written to it (write_if_built = 0 skips that,
 * e.g. on the second and later devices of a multi-GPU host).  *status (may be NULL): bit 0 / 1 = racg / racs read from
 * file, bit 2 / 3 = racg / racs written.  A missing directory is not an error here (the reference aborts, M:3718):
 * nothing is written.  No-op for an iiwarm context (M:773). */
int kidmp_table_cache_reuse(kidmp_ctx *ctx, const char *dir, int32_t l_reuse, int32_t write_if_built, int32_t *status);
/* The same format on host buffers (no GPU needed): ntab arrays of n_each doubles, Fortran element order. */
int kidmp_cache_write_file(const char *path, int32_t ntab, const double *const *tabs, int64_t n_each);
int kidmp_cache_read_file(const char *path, int32_t ntab, double *const *tabs, int64_t n_each);

/* Diagnostics: evaluate one of the column kernel's own fp64 math helpers (kid_amd/csrc/fastmath.h, which stand
 * in for the reference's DLOG / ALOG10 / EXP / 10.**x / x**y / SQRT / x**(1./3.)) on the device, elementwise on
 * host arrays: out[i] = fn(x[i]) (fn(x[i], y[i]) for KIDMP_MATH_POW; y is read but ignored otherwise). */
#define KIDMP_MATH_LOG    0
#define KIDMP_MATH_LOG10  1
#define KIDMP_MATH_EXP    2
#define KIDMP_MATH_EXP10  3
#define KIDMP_MATH_SQRT   4
#define KIDMP_MATH_CBRT   5
#define KIDMP_MATH_POW    6
#define KIDMP_MATH_RCP_SEED 7  /* raw v_rcp_f64(y)                                  */
#define KIDMP_MATH_DIV    8    /* the kernel's x / y (seed, one Newton step, residual correction) */
#define KIDMP_MATH_IEEE_DIV 9  /* IEEE x / y, for comparison                        */
#define KIDMP_MATH_RCP    10   /* the kernel's 1 / y (seed, one cubically convergent step) */
int kidmp_math_probe(kidmp_ctx *ctx, int32_t fn, int64_t n, const double *x, const double *y, double *out);
/* The same on three operands and in either arithmetic, from a unit compiled with the column kernel's own flags (so its
 * plain division is the kernel's binary32 one).  fn: the codes above, unchanged in meaning, and the ones below.
 * binary32 != 0: every operand is narrowed to float (exact when the caller passes binary32-representable values), the
 * float overload of fastmath.h is evaluated and the result widened; KIDMP_MATH_RCP_SEED is then the raw v_rcp_f32.
 * KIDMP_MATH_DIV, KIDMP_MATH_IEEE_DIV, KIDMP_MATH_RCP and the two mixed-type powers exist in binary64 only: KIDMP_EINVAL with binary32 != 0.
 * All arrays are host arrays of n doubles and all four are required, whichever of them fn reads. */
#define KIDMP_MATH_POW10_TIMES_POW 11  /* 10**x * y**z in one exponential (pow10_times_pow(x, log2_parts(y), z)) */
#define KIDMP_MATH_PLAIN_DIV 12        /* x / y as the column kernel's flags compile it                           */
#define KIDMP_MATH_PLAIN_RCP 13        /* 1 / y likewise                                                          */
#define KIDMP_MATH_POW_DF    14        /* pow(double x, float y): DOUBLE**REAL, evaluated in binary64             */
#define KIDMP_MATH_POW_FD    15        /* pow(float x, double y): REAL**DOUBLE, evaluated in binary64             */
/* A size-limit test of the scheme decided both ways (kid_amd/csrc/limit_bracket.h), binary64 only: x = num, y = den,
 * z = the site (0: ice, 1: rain, 2 .. 15: cloud droplets with nu = z).  out = b + 4 * o + 16 * i, where b is the bracket's
 * answer (0 below, 1 inside, 2 above, 3 ambiguous), o the decision of the column kernel's original expression
 * c / root3(num / den) against the two limits (0, 1 or 2) and i the one-sided form the kernel votes on
 * (1: certainly inside).  Not a function of fastmath.h: the codes from 32 on are decisions of the kernel;
 * 16 .. 31 stay unassigned (KIDMP_EINVAL). */
#define KIDMP_MATH_LIMIT_BRACKET 32
int kidmp_math_probe_ex(kidmp_ctx *ctx, int32_t fn, int32_t binary32, int64_t n, const double *x, const double *y,
                        const double *z, double *out);

/* Seconds spent in table construction during kidmp_init (host wall clock). */
double kidmp_init_seconds(const kidmp_ctx *ctx);

/* Name of the column-step kernel as it appears in rocprofv3 traces. */
const char *kidmp_kernel_name(void);

/* Identifies the code object of this context's nz <= 120 column-step kernel:
 * "src:<hash of the kernel sources and flags>;vgpr:<n>;lds:<bytes>;scratch:<bytes>".  Profiles under profiles/
 * carry it, so a counter file measured on another build of the kernel is recognised as stale (bench.py). */
const char *kidmp_kernel_fingerprint(kidmp_ctx *ctx);
/* The same for the binary32 code objects behind kidmp32_*: arith = KIDMP_ARITH_P32N or KIDMP_ARITH_F32 ("" otherwise). */
const char *kidmp32_kernel_fingerprint(kidmp_ctx *ctx, int32_t arith);

#ifdef __cplusplus
}
#endif
#endif /* KIDMP_H */
