/* Stand-alone check of the oracle's schedule entry (orc_maketreelistMCMC_schedule): on a ladder tree built here, the updating
 * driver's run is reproduced bit for bit by a run that is handed the models orc_qupdate_apply makes of the driver's own rows --
 * hidden rates at n = 8 (KS) and two states (BF).  Built with the host compiler and -fsanitize=address,undefined together with
 * oracle/phm_oracle.c by tests/test_rate_updates_cpu.py, and run on its own.  Prints "ok" and returns 0 when everything holds. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "phm_oracle.h"

#define T 24                 /* tips */
#define E (2 * (T - 1))
#define NIT 10

static int fail(const char* what) { printf("FAILED: %s\n", what); return 1; }

static int run_case(int n, int variant, const double* Q_rm, double Omega, const double* prior) {
  const int kk = (variant == ORC_MCMC_KS) ? n / 2 - 1 : 0;
  const int cols = n + n * n + 2 + 3 * kk + 1;
  /* ladder: internal node T+1+i holds tip i+1 and the next internal node; the last one holds tips T-1 and T */
  int32_t edge[2 * E], states[T], map_off[E + 1], mapnames[2 * E], nen[E], nodelist[T - 2];
  double maps[2 * E];
  for (int i = 0; i < T - 1; ++i) {
    edge[2 * i] = T + 1 + i;     edge[E + 2 * i] = i + 1;
    edge[2 * i + 1] = T + 1 + i; edge[E + 2 * i + 1] = (i < T - 2) ? T + 2 + i : T;
  }
  for (int t = 0; t < T; ++t) states[t] = 1 + (t * 7 % 5 < 2);
  for (int b = 0; b < E; ++b) {
    const int child = edge[E + b];
    const double len = 0.3 + 0.05 * (b % 7);
    map_off[b] = 2 * b;
    maps[2 * b] = maps[2 * b + 1] = len / 2;
    mapnames[2 * b] = 1; mapnames[2 * b + 1] = (child <= T) ? states[child - 1] : 1;
  }
  map_off[E] = 2 * E;
  for (int i = 0; i < T - 1; ++i) { nen[2 * i] = 2 * (T - 2 - i) + 1; nen[2 * i + 1] = 2 * (T - 2 - i) + 2; }   /* deepest node first */
  for (int i = 0; i < T - 2; ++i) nodelist[i] = T + 2 + i;                                                      /* root side first */
  orc_tree x = { T, T - 1, E, edge, NULL, states, map_off, maps, mapnames };

  double *Qcm = malloc(sizeof(double) * n * n), *Bcm = malloc(sizeof(double) * n * n), *pid = malloc(sizeof(double) * n);
  for (int i = 0; i < n; ++i) {
    pid[i] = 1.0 / n;
    for (int j = 0; j < n; ++j) { Qcm[i + j * n] = Q_rm[i * n + j]; Bcm[i + j * n] = (i == j ? 1.0 : 0.0) + Q_rm[i * n + j] / Omega; }
  }
  double *want = malloc(sizeof(double) * NIT * cols), *got = malloc(sizeof(double) * NIT * cols);
  double *sched = malloc(sizeof(double) * NIT * n * n), *row = malloc(sizeof(double) * cols);
  orc_rng rng; memset(&rng, 0, sizeof rng); rng.seed_lo = 7; rng.seed_hi = 5; rng.replica = 3;
  int bad = 0;
  if (orc_maketreelistMCMC_qupdate(&x, n, Qcm, pid, Bcm, Omega, nen, nodelist, T + 1, NIT, variant, prior, 0, &rng, want, NULL))
    bad = fail("the updating driver's status");
  memcpy(sched, Q_rm, sizeof(double) * n * n);
  int changed = 0;
  for (int it = 0; it + 1 < NIT && !bad; ++it) {
    double* next = sched + (size_t)(it + 1) * n * n;
    memcpy(next, next - n * n, sizeof(double) * n * n);
    for (int c = 0; c < cols; ++c) row[c] = want[(size_t)c * NIT + it];
    if (orc_qupdate_apply(variant, n, next, Omega, prior, row, rng.seed_lo, rng.seed_hi, (uint32_t)it)) bad = fail("orc_qupdate_apply");
    changed += memcmp(next, next - n * n, sizeof(double) * n * n) != 0;
  }
  if (!bad && changed < NIT / 2) bad = fail("the models hardly change");
  if (!bad && orc_maketreelistMCMC_schedule(&x, n, sched, pid, Bcm, Omega, nen, nodelist, T + 1, NIT, variant, 0, &rng, got, NULL))
    bad = fail("the schedule entry's status");
  if (!bad && memcmp(got, want, sizeof(double) * NIT * cols)) bad = fail("the scheduled run differs from the updating run");
  /* refusals: a variant without parameter columns, a sequential random stream, no schedule */
  if (!bad && orc_maketreelistMCMC_schedule(&x, n, sched, pid, Bcm, Omega, nen, nodelist, T + 1, NIT, ORC_MCMC_PLAIN, 0, &rng, got, NULL) != ORC_ERR_BAD_INPUT)
    bad = fail("PLAIN accepted");
  orc_rng seq = rng; seq.mode = 2;
  if (!bad && orc_maketreelistMCMC_schedule(&x, n, sched, pid, Bcm, Omega, nen, nodelist, T + 1, NIT, variant, 0, &seq, got, NULL) != ORC_ERR_BAD_INPUT)
    bad = fail("R-stream mode accepted");
  if (!bad && orc_maketreelistMCMC_schedule(&x, n, NULL, pid, Bcm, Omega, nen, nodelist, T + 1, NIT, variant, 0, &rng, got, NULL) != ORC_ERR_BAD_INPUT)
    bad = fail("NULL schedule accepted");
  free(row); free(sched); free(got); free(want); free(pid); free(Bcm); free(Qcm);
  return bad;
}

int main(void) {
  /* hidden rates, n = 8: l01 = 0.05, l10 = 0.08, three regimes (synth.make2sQ's layout) */
  enum { N8 = 8 };
  static double Q8[N8 * N8];
  const double rk[3] = { 0.02, 0.03, 0.04 }, lk[3] = { 0.03, 0.04, 0.05 }, gm[3] = { 0.5, 0.75, 1.0 };
  Q8[0 * N8 + 1] = 0.05; Q8[1 * N8 + 0] = 0.08;
  for (int i = 1; i <= 3; ++i) {
    Q8[(2 * i - 2) * N8 + 2 * i] = rk[i - 1]; Q8[(2 * i - 1) * N8 + 2 * i + 1] = rk[i - 1];
    Q8[(2 * i) * N8 + 2 * i - 2] = lk[i - 1]; Q8[(2 * i + 1) * N8 + 2 * i - 1] = lk[i - 1];
    Q8[(2 * i) * N8 + 2 * i + 1] = gm[i - 1] * 0.05; Q8[(2 * i + 1) * N8 + 2 * i] = gm[i - 1] * 0.08;
  }
  double qmax = 0;
  for (int i = 0; i < N8; ++i) {
    double s = 0;
    for (int j = 0; j < N8; ++j) if (j != i) s += Q8[i * N8 + j];
    Q8[i * N8 + i] = -s;
    if (s > qmax) qmax = s;
  }
  const double prior_ks[6] = { 1, 10, 2, 10, 20, 2 }, prior_bf[4] = { .55, 1, .56, 1.01 };
  const double Q2[4] = { -.1, .1, .1, -.1 };
  if (run_case(N8, ORC_MCMC_KS, Q8, 4.0 * qmax, prior_ks)) return 1;
  if (run_case(2, ORC_MCMC_BF, Q2, 10.0, prior_bf)) return 1;
  printf("ok\n");
  return 0;
}
