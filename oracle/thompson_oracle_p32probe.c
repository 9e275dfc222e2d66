/*
 * thompson_oracle_p32probe.c -- CPU ORACLE (test infrastructure, NOT product code).
 *
 * A PROBE build of the P32n arithmetic (thompson_oracle_p32n.c): thompson_oracle_column.c once more under -DTH_P32N,
 * with the special functions routed through the helpers below, so that the oracle itself can say at which levels the
 * last bits of a special function decide the result (tests/parity32.py).  Entry points carry the suffix _p32probe and
 * live beside the _p32n ones in one library; they read the view that the unmodified P32n build made
 * (th_oracle_make_view_p32probe exists and is never called).
 *
 * What the helpers do, selected by th_oracle_probe_set(shift, pattern, narrow), which is called BETWEEN batches only
 * (the settings are plain globals that the workers read):
 *   REAL arguments     exp, log, log10, cbrt, pow (every argument REAL; where <tgmath.h> picks expf, powf, ...) are
 *                      evaluated in binary64, rounded once to binary32 and then moved by `shift` ulp (signed, towards
 *                      +inf for a positive shift).  pattern 0: every call by +shift; 1: every call by -shift;
 *                      2: alternating by call, +shift first, restarting with every column (so a batch does not depend
 *                      on which worker steps which column).  Zeros, infinities and NaNs are not moved, and a move never
 *                      crosses zero or reaches infinity.
 *   REAL reciprocals   the `1. / x` of mp_thompson (RCP in thompson_oracle_column.c: odt, orho, ocp, otemp, odzq, the
 *                      inverse slopes ...) with a REAL x are moved in the same way.  A device forms them with its
 *                      reciprocal unit (1 ulp), not with a correctly rounded division, and they decide what is left of
 *                      a species that a process removes completely: qc1d + qcten*DT with qcten = -rc*orho*odt is 0 or
 *                      one ulp of qc1d (3e-11 > R1, with a droplet number of its own) depending on the last bit of orho.
 *                      Moving only odt and orho gives the same spreads to the second digit: they are what matters.
 *   REAL rate limiters the six quotients ratio = rate_max / sump of block I (RDIV) are moved in the same way: they scale a
 *                      species' sinks so that exactly everything is removed, and decide the same 0-or-one-ulp residue
 *                      (seen on the device at 236 ... 242 K, cloud water rimed and frozen away completely).
 *                      Other REAL quotients a / b are NOT moved.
 *   DOUBLE arguments   the same five functions are glibc's binary64 ones; with narrow != 0 their result is rounded to
 *                      binary32 (and widened again), which is what an all-binary32 build makes of the rates' special
 *                      functions.  sqrt is correctly rounded in every build and stays <tgmath.h>'s.
 * With shift 0 and narrow 0 the build differs from thompson_oracle_p32n.c only where glibc's binary32 function does not
 * return the correctly rounded result (tests/test_parity32.py).
 *
 * No floating-point literal below: this file is compiled with -fsingle-precision-constant like the other P32n build.
 */
#define TH_P32N 1
#define TH_PROBE 1
#include <math.h>
#include <tgmath.h>

static int probe_shift, probe_pattern, probe_narrow;
static _Thread_local unsigned probe_calls;

void th_oracle_probe_set(int shift, int pattern, int narrow)
{
    probe_shift = shift; probe_pattern = pattern; probe_narrow = narrow;
}
#define TH_PROBE_COLUMN_START() (probe_calls = 0)

/* y: the binary64 evaluation of a REAL-argument function */
static float probe_round(double y)
{
    float r = (float)y;
    int s = probe_shift;
    if (s == 0 || !isfinite(r) || r == 0) return r;
    if (probe_pattern == 1) s = -s;
    else if (probe_pattern == 2 && (probe_calls++ & 1u)) s = -s;
    const float to = s > 0 ? INFINITY : -INFINITY;
    for (int i = s > 0 ? s : -s; i > 0; i--) {
        const float q = nextafterf(r, to);
        if (!isfinite(q) || q == 0) break;
        r = q;
    }
    return r;
}
static inline double probe_wide(double y) { return probe_narrow ? (double)(float)y : y; }

static inline float  probe_exp_r(float x)            { return probe_round((exp)((double)x)); }
static inline float  probe_log_r(float x)            { return probe_round((log)((double)x)); }
static inline float  probe_log10_r(float x)          { return probe_round((log10)((double)x)); }
static inline float  probe_cbrt_r(float x)           { return probe_round((cbrt)((double)x)); }
static inline float  probe_pow_r(float x, float y)   { return probe_round((pow)((double)x, (double)y)); }
static inline float  probe_rcp_r(float x)            { return probe_round((double)1 / (double)x); }   /* exact to the last bit at shift 0: 53 >= 2*24 + 2 */
static inline float  probe_div_r(float a, float b)   { return probe_round((double)a / (double)b); }     /* the same at shift 0 */
static inline double probe_div_d(double a, double b) { return a / b; }
static inline double probe_rcp_d(double x)           { return (double)1 / x; }
static inline double probe_exp_d(double x)           { return probe_wide((exp)(x)); }
static inline double probe_log_d(double x)           { return probe_wide((log)(x)); }
static inline double probe_log10_d(double x)         { return probe_wide((log10)(x)); }
static inline double probe_cbrt_d(double x)          { return probe_wide((cbrt)(x)); }
static inline double probe_pow_d(double x, double y) { return probe_wide((pow)(x, y)); }

/* the type rules of <tgmath.h>: binary32 only where every argument is REAL, binary64 otherwise (integers included) */
#undef exp
#undef log
#undef log10
#undef cbrt
#undef pow
#define exp(x)    _Generic((x), float: probe_exp_r, default: probe_exp_d)(x)
#define log(x)    _Generic((x), float: probe_log_r, default: probe_log_d)(x)
#define log10(x)  _Generic((x), float: probe_log10_r, default: probe_log10_d)(x)
#define cbrt(x)   _Generic((x), float: probe_cbrt_r, default: probe_cbrt_d)(x)
#define RCP(x)    _Generic((x), float: probe_rcp_r, default: probe_rcp_d)(x)
#define RDIV(a, b) _Generic((a), float: _Generic((b), float: probe_div_r, default: probe_div_d), default: probe_div_d)(a, b)
#define pow(x, y) _Generic((x), float: _Generic((y), float: probe_pow_r, default: probe_pow_d), default: probe_pow_d)(x, y)

#include "thompson_oracle_column.c"
