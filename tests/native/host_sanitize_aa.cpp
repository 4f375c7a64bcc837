// Host-only sanitizer driver (AddressSanitizer + UndefinedBehaviorSanitizer) for the host core of Anderson acceleration
// (scs_amd/csrc/aa_small.h) through the host path that uses all of it (aa_host.cpp): weight-capped, rank-0 and zero-gamma
// solves under both types at dim = 40 -- the settings of tests/test_aa_dev_gpu.py (REJ_SETTINGS) -- and one run whose steps
// are accepted, with relaxation and a memory larger than dim allows.  Test infrastructure; built by tests/test_aa_host.py
// with hipcc --cuda-host-only.
#include "../../scs_amd/csrc/aa_host.cpp"
#include <random>
using namespace scsamd;

static int run(int type1, real reg, int mem, real relax, real cap, bool identity, unsigned seed, AaStats *st) {
  const int dim = 40, iters = 50;
  std::mt19937 rng(seed);
  std::uniform_real_distribution<double> u(0, 1);
  std::normal_distribution<double> nd;
  std::vector<real> d0(dim), d1(dim), c(dim), x(dim), xp(dim), fx(dim);
  for (int i = 0; i < dim; ++i) {
    d0[i] = (real)(0.3 + 0.65 * u(rng));
    d1[i] = (real)(-0.02 + 0.04 * u(rng));
    c[i] = (real)nd(rng);
    x[i] = (real)nd(rng);
  }
  AaHost *a = aa_host_init(dim, mem, mem, type1, reg, relax, 1.0, cap, 5);
  if (!a) return 1;
  xp = x;
  for (int it = 0; it < iters; ++it) {
    if (it > 0) {
      const real nrm = aa_host_apply(x.data(), xp.data(), a);
      if (std::isnan((double)nrm)) return 2;
    }
    xp = x;
    for (int i = 0; i < dim; ++i)
      fx[i] = identity ? xp[i] : d0[i] * xp[i] + d1[i] * xp[(i + dim - 1) % dim] + c[i] + (real)0.03 * std::max(xp[i], (real)0);
    x = fx;
    aa_host_safeguard(x.data(), xp.data(), a);
    for (int i = 0; i < dim; ++i)
      if (!std::isfinite((double)x[i])) return 3;
  }
  aa_host_stats(a, st);
  aa_host_reset(a);
  aa_host_finish(a);
  return 0;
}

int main() {
  struct Case {
    int type1;
    real reg;
    int mem;
    real relax, cap;
    bool identity;
  };
  const Case cases[] = {
      {0, (real)1e-12, 5, 1, (real)0.5, false}, {0, (real)1e-12, 5, 1, (real)0.5, true}, // A: weight cap; rank 0
      {1, (real)-1e-6, 4, 1, (real)0.5, false}, {1, (real)-1e-6, 4, 1, (real)0.5, true}, // B: weight cap; gamma == 0
      {1, (real)1e-8, 64, (real)1.3, (real)1e10, false},                                 // accepted steps, mem cut to dim
  };
  int n = 0;
  for (const Case &k : cases) {
    AaStats st;
    const int rc = run(k.type1, k.reg, k.mem, k.relax, k.cap, k.identity, 100 + n, &st);
    if (rc) {
      printf("case %d failed (%d)\n", n, rc);
      return 1;
    }
    printf("case %d: iter %d accept %d lapack %d rank0 %d nonfinite %d cap %d safeguard %d last_rank %d\n", n, (int)st.iter,
           (int)st.n_accept, (int)st.n_reject_lapack, (int)st.n_reject_rank0, (int)st.n_reject_nonfinite,
           (int)st.n_reject_weight_cap, (int)st.n_safeguard_reject, (int)st.last_rank);
    const bool capped = n == 0 || n == 2;
    if (n < 4 && (st.n_accept != 0 || (capped && st.n_reject_weight_cap == 0) || (n == 1 && st.n_reject_rank0 == 0))) {
      printf("case %d did not take the path it is here for\n", n);
      return 1;
    }
    if (n == 4 && st.n_accept == 0) {
      printf("case %d accepted nothing\n", n);
      return 1;
    }
    ++n;
  }
  if (aa_host_init(40, 5, 0, 1, (real)1e-8, 1, 1, 1, 5) || aa_host_init(40, 5, 5, 1, (real)1e-8, 3, 1, 1, 5)) return 1;
  AaHost *z = aa_host_init(40, 0, 0, 1, (real)1e-8, 1, 1, 1, 5); // no memory: every call returns 0
  std::vector<real> v(40, 1), w(40, 2);
  if (!z || aa_host_apply(v.data(), w.data(), z) != 0 || aa_host_safeguard(v.data(), w.data(), z) != 0) return 1;
  aa_host_finish(z);
  printf("sanitizer driver ok\n");
  return 0;
}
