// nais_geo_cr.h -- sin, cos and acos of a double rounded from a double-double evaluation, so that
// they agree with a host libm that rounds (almost always) correctly. The device libm's functions
// are good to an ulp or two, which is enough everywhere but in powerLaw.dist for POIs a few
// hundred metres apart: d = R acos(c) turns a last-bit difference of c into 2^-53 / angle^2 of d
// (about 120 float32 ulps at 25 m). The batch builder of GeoIE hands such distances to the model
// as the reference's dist_mat holds them, so it evaluates the formula with these.
//
// Double-double: a value is the unevaluated sum h + l of two doubles, |l| <= ulp(h) / 2
// (Dekker / Knuth error-free transforms; the products' errors come from fma).
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define NAIS_CR_HD __host__ __device__ inline
#else
#define NAIS_CR_HD inline
#endif

// The error-free transforms hold only if every + and * rounds on its own. hipcc contracts a
// product into the add that uses it, also across inlined calls (s = x + (-(k * P1)) becomes one
// fma and two_sum's error term is then wrong), so every function here switches contraction off.
#if defined(__clang__)
#define NAIS_CR_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define NAIS_CR_NO_CONTRACT
#endif

namespace nais_geo_cr {

struct DD {
  double h, l;
};

NAIS_CR_HD DD quick_two_sum(double a, double b) {   // |a| >= |b|
  NAIS_CR_NO_CONTRACT
  const double s = a + b;
  return DD{s, b - (s - a)};
}

NAIS_CR_HD DD two_sum(double a, double b) {
  NAIS_CR_NO_CONTRACT
  const double s = a + b, bb = s - a;
  return DD{s, (a - (s - bb)) + (b - bb)};
}

NAIS_CR_HD DD two_prod(double a, double b) {
  NAIS_CR_NO_CONTRACT
  const double p = a * b;
  return DD{p, fma(a, b, -p)};
}

NAIS_CR_HD DD dd_add(DD a, DD b) {
  NAIS_CR_NO_CONTRACT
  DD s = two_sum(a.h, b.h);
  const DD t = two_sum(a.l, b.l);
  s = quick_two_sum(s.h, s.l + t.h);
  return quick_two_sum(s.h, s.l + t.l);
}

NAIS_CR_HD DD dd_neg(DD a) { return DD{-a.h, -a.l}; }

NAIS_CR_HD DD dd_mul(DD a, DD b) {
  NAIS_CR_NO_CONTRACT
  const DD p = two_prod(a.h, b.h);
  return quick_two_sum(p.h, p.l + (a.h * b.l + a.l * b.h));
}

NAIS_CR_HD DD dd_div_d(DD a, double b) {
  NAIS_CR_NO_CONTRACT
  const double q1 = a.h / b;
  const DD r = dd_add(a, dd_neg(two_prod(q1, b)));
  return quick_two_sum(q1, r.h / b);
}

// sin and cos of x (|x| < 1e5) to about 2^-100: x = k pi/2 + r with pi/2 in three doubles, then
// the Taylor series of sin r and cos r (|r| <= pi/4: the 14th terms are below 1e-31), each only
// if `need` asks for the result it feeds (1: *s, 2: *c) and until its terms fall below the
// double-double resolution of its sum
NAIS_CR_HD void sincos_dd(double x, DD* s, DD* c, int need) {
  NAIS_CR_NO_CONTRACT
  const double P1 = 1.5707963267948966, P2 = 6.123233995736766e-17, P3 = -1.4973849048591698e-33;
  const double k = rint(x * 0.6366197723675814);
  const int q = int(k) & 3;
  DD r = dd_add(DD{x, 0.0}, dd_neg(two_prod(k, P1)));
  r = dd_add(r, dd_neg(two_prod(k, P2)));
  r = dd_add(r, DD{-k * P3, 0.0});
  const DD r2 = dd_mul(r, r);
  DD ts = r, ss = r, tc = DD{1.0, 0.0}, sc = tc;
  bool go_s = (need & ((q & 1) ? 2 : 1)) != 0, go_c = (need & ((q & 1) ? 1 : 2)) != 0;
  for (int n = 1; n <= 13 && (go_s || go_c); ++n) {
    if (go_c) {
      tc = dd_div_d(dd_mul(tc, r2), -double((2 * n - 1) * (2 * n)));
      sc = dd_add(sc, tc);
      go_c = fabs(tc.h) > 1e-34 * fabs(sc.h);
    }
    if (go_s) {
      ts = dd_div_d(dd_mul(ts, r2), -double((2 * n) * (2 * n + 1)));
      ss = dd_add(ss, ts);
      go_s = fabs(ts.h) > 1e-34 * fabs(ss.h);
    }
  }
  switch (q) {
    case 0: *s = ss; *c = sc; break;
    case 1: *s = sc; *c = dd_neg(ss); break;
    case 2: *s = dd_neg(ss); *c = dd_neg(sc); break;
    default: *s = dd_neg(sc); *c = ss; break;
  }
}

NAIS_CR_HD double cr_sin(double x) {
  NAIS_CR_NO_CONTRACT
  if (!(fabs(x) < 1e5)) return sin(x);
  DD s, c;
  sincos_dd(x, &s, &c, 1);
  return s.h;
}

NAIS_CR_HD double cr_cos(double x) {
  NAIS_CR_NO_CONTRACT
  if (!(fabs(x) < 1e5)) return cos(x);
  DD s, c;
  sincos_dd(x, &s, &c, 2);
  return c.h;
}

// acos: one Newton step on cos y = c from the libm's value, the residual in double-double
NAIS_CR_HD double cr_acos(double x) {
  NAIS_CR_NO_CONTRACT
  const double y = acos(x);
  if (!(fabs(x) < 1.0)) return y;
  DD s, c;
  sincos_dd(y, &s, &c, 2);   // the divisor needs no more than the libm's sine
  const DD d = dd_add(c, DD{-x, 0.0});
  return y + (d.h + d.l) / sin(y);
}

}  // namespace nais_geo_cr
