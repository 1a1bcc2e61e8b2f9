// TEST INFRASTRUCTURE ONLY -- replays the oracle's variates through the reference's own
// compiled retstable_LD (Code/C/retstable.cpp, built untouched by `make ref`; its RNG is
// the tape player of ref_shim/RNG.hpp).  See oracle/ref.py and DESIGN.md s3.
//
// Per draw (h, alpha, V0, key, t, j): bbo_retstable_tape (bb_oracle.c) lists the variates
// of the oracle's Philox blocks in the order retstable_LD asks for them; retstable_LD then
// draws from that tape.  Reported: its value, the items it consumed and a flag word.
#include <cstdint>
#include <stdexcept>
#include <vector>

#include "retstable.h"

extern "C" {
double bbo_retstable_tape(double h, double alpha, double V0, const uint64_t key[2], uint64_t t,
                          uint64_t j, int *kind, double *value, long cap, long *inner_per_outer,
                          long cap_outer, long *n_items, long *n_outer, long *n_inner);
}

enum {
  BBR_KIND_MISMATCH = 1,  // an item was served to another kind of call than it was made for
  BBR_EXHAUSTED = 2,      // retstable_LD asked past the end of the tape
  BBR_LEFTOVER = 4,       // retstable_LD returned with items left
  BBR_TAPE_CUT = 8,       // the oracle's draw needs more items than TAPE_CAP
};

static const long TAPE_CAP = 1 << 16;
static const long OUTER_CAP = 1 << 12;

static int replay(double h, double alpha, double V0, const int *kind, const double *value, long n,
                  double *x, long *consumed)
{
  RNG r(kind, value, n);
  int flags = 0;
  *x = 0.0;
  try {
    *x = retstable_LD(h, alpha, r, V0);
  } catch (const std::out_of_range &) {
    flags |= BBR_EXHAUSTED;
  }
  if (r.mismatches) flags |= BBR_KIND_MISMATCH;
  if (!(flags & BBR_EXHAUSTED) && r.pos != n) flags |= BBR_LEFTOVER;
  *consumed = r.pos;
  return flags;
}

extern "C" {

// retstable_LD on a tape given by the caller (the shim's self-test).
int bbr_replay(double h, double alpha, double V0, const int *kind, const double *value, long n,
               double *x, long *consumed)
{
  return replay(h, alpha, V0, kind, value, n, x, consumed);
}

// Draw i on counters (t[i], j[i]) under one key: x_ref from retstable_LD, x_oracle from
// bbo_retstable_tape, the items the oracle listed (n_items) and the reference consumed,
// the oracle's outer / inner attempts, and the flag word (0: kinds matched and the tape was
// consumed exactly).
void bbr_retstable_batch(long num, const double *h, const double *alpha, const double *V0,
                         const uint64_t key[2], const uint64_t *t, const uint64_t *j,
                         double *x_ref, double *x_oracle, long *n_items, long *consumed,
                         long *n_outer, long *n_inner, int *flags)
{
  std::vector<int> kind(TAPE_CAP);
  std::vector<double> value(TAPE_CAP);
  std::vector<long> ipo(OUTER_CAP);
  for (long i = 0; i < num; ++i) {
    x_oracle[i] = bbo_retstable_tape(h[i], alpha[i], V0[i], key, t[i], j[i], kind.data(),
                                     value.data(), TAPE_CAP, ipo.data(), OUTER_CAP, &n_items[i],
                                     &n_outer[i], &n_inner[i]);
    if (n_items[i] > TAPE_CAP) {
      flags[i] = BBR_TAPE_CUT;
      x_ref[i] = 0.0;
      consumed[i] = 0;
      continue;
    }
    flags[i] = replay(h[i], alpha[i], V0[i], kind.data(), value.data(), n_items[i], &x_ref[i],
                      &consumed[i]);
  }
}

// lambda | beta, tau of BridgeRegression.cpp:509 around the reference call, coefficient j on
// counters (t, j0 + j).
void bbr_lambda_batch(long p, const double *beta, double alpha, double tau, const uint64_t key[2],
                      uint64_t t, uint64_t j0, double *lam_ref, double *lam_oracle,
                      long *n_outer, long *n_inner, int *flags)
{
  std::vector<int> kind(TAPE_CAP);
  std::vector<double> value(TAPE_CAP);
  std::vector<long> ipo(OUTER_CAP);
  for (long j = 0; j < p; ++j) {
    double h = beta[j] * beta[j] / (tau * tau), a = 0.5 * alpha;
    long n = 0;
    lam_oracle[j] = 2 * bbo_retstable_tape(h, a, 1.0, key, t, j0 + (uint64_t)j, kind.data(),
                                           value.data(), TAPE_CAP, ipo.data(), OUTER_CAP, &n,
                                           &n_outer[j], &n_inner[j]);
    if (n > TAPE_CAP) {
      flags[j] = BBR_TAPE_CUT;
      lam_ref[j] = 0.0;
      continue;
    }
    // retstable.h's default V0 is 1.0: the call of BridgeRegression.cpp:509
    long used = 0;
    flags[j] = replay(h, a, 1.0, kind.data(), value.data(), n, &lam_ref[j], &used);
    lam_ref[j] = 2 * lam_ref[j];
  }
}

}  // extern "C"
