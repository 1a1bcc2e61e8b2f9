// TEST INFRASTRUCTURE ONLY -- stand-in for the RNG class that the reference's
// Code/C/retstable.h includes and does not ship.  It is a tape player: it serves a
// prepared list of variates, one per call, and knows nothing of the sampler that asks.
//
// retstable.cpp uses three members: unif(), norm(mu, sd), expon_rate(rate).  Each tape
// item carries the kind of call it was prepared for; serving it to another kind is noted
// in `mismatches` (the value is served all the same).  Asking past the end throws: a
// wrong tape must end the reference's rejection loops, not spin them for ever.
#ifndef BB_REF_SHIM_RNG_HPP
#define BB_REF_SHIM_RNG_HPP

#include <stdexcept>

class RNG {
public:
  enum Kind { UNIF = 0, NORM = 1, EXPON = 2, ANY = 3 };  // ANY: whatever is asked

  const int *kind;
  const double *value;
  long n, pos, mismatches;

  RNG(const int *kind_, const double *value_, long n_)
      : kind(kind_), value(value_), n(n_), pos(0), mismatches(0) {}

  double unif() { return next(UNIF); }
  double norm(double mu, double sd) { return mu + sd * next(NORM); }
  double expon_rate(double rate) { return next(EXPON) / rate; }

private:
  double next(int asked) {
    if (pos >= n) throw std::out_of_range("RNG tape exhausted");
    if (kind[pos] != ANY && kind[pos] != asked) ++mismatches;
    return value[pos++];
  }
};

#endif
