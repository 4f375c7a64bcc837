// Host-only sanitizer driver (AddressSanitizer + UndefinedBehaviorSanitizer) for the host half of scs_amd_update_matrix
// (scs_amd/csrc/reorder.cpp): the entry permutation recorded with the renumbering -- by both ways scs_init comes by the renumbered
// matrix --, the finiteness check and the value permutation.  Random patterns with mixed cones as in host_sanitize_reorder.cpp, plus
// the edges: columns without entries, a matrix without any entry, and entry positions at the top of the `eoff` range (arithmetic only:
// nothing of that size is allocated).  Test infrastructure; built by tests/test_update_matrix_cpu.py with hipcc --cuda-host-only.
#include "../../scs_amd/csrc/reorder.cpp"
#include <limits>
#include <random>
using namespace scsamd;

static int fail(const char *what, int trial) {
  printf("FAILED: %s (trial %d)\n", what, trial);
  return 1;
}

// B = A[row_new2old][:, col_new2old] with sorted rows, and entry_new2old names the source of every entry: checked entry by entry
static int check(const HostCsc &A, const HostCsc &B, const Reorder &R, int trial) {
  const size_t nnz = A.x.size();
  if (!R.active) return 0;
  if (R.entry_new2old.size() != nnz) return fail("entry permutation has the wrong length", trial);
  std::vector<int> row_old2new((size_t)A.m);
  for (int i = 0; i < A.m; ++i) row_old2new[R.row_new2old[i]] = i;
  std::vector<char> seen(nnz, 0);
  for (int j = 0; j < A.n; ++j) {
    const int jo = R.col_new2old[j];
    if (B.p[j + 1] - B.p[j] != A.p[jo + 1] - A.p[jo]) return fail("column length", trial);
    for (eoff o = B.p[j]; o < B.p[j + 1]; ++o) {
      const eoff q = R.entry_new2old[(size_t)o];
      if (q < A.p[jo] || q >= A.p[jo + 1]) return fail("entry maps outside its column", trial);
      if (seen[(size_t)q]) return fail("entry used twice", trial);
      seen[(size_t)q] = 1;
      if (row_old2new[A.i[(size_t)q]] != B.i[(size_t)o]) return fail("entry maps to another row", trial);
      if (A.x[(size_t)q] != B.x[(size_t)o]) return fail("value did not follow its entry", trial);
      if (o > B.p[j] && B.i[(size_t)o - 1] > B.i[(size_t)o]) return fail("rows not sorted", trial);
    }
  }
  // new values through the same permutation
  std::vector<real> nx(nnz), out(nnz, (real)-1);
  for (size_t q = 0; q < nnz; ++q) nx[q] = (real)(3 * q + 1);
  if (!all_finite(nx.data(), nnz)) return fail("finite values reported as not finite", trial);
  permute_values(R, nx.data(), nnz, out.data());
  for (size_t o = 0; o < nnz; ++o)
    if (out[o] != nx[(size_t)R.entry_new2old[o]]) return fail("permute_values", trial);
  if (nnz) {
    nx[nnz / 2] = std::numeric_limits<real>::quiet_NaN();
    if (all_finite(nx.data(), nnz)) return fail("NaN not seen", trial);
    nx[nnz / 2] = 0;
    nx[nnz - 1] = -std::numeric_limits<real>::infinity();
    if (all_finite(nx.data(), nnz)) return fail("inf in the last entry not seen", trial);
  }
  return 0;
}

int main() {
  std::mt19937 rng(11);
  int kept = 0, ready = 0;
  for (int trial = 0; trial < 40; ++trial) {
    const int n = trial == 0 ? 120000 : 50 + rng() % 3000, cn = trial == 0 ? 10 : 2 + rng() % 9;
    std::vector<long long> q;
    int z = trial == 0 ? 30000 : rng() % 200, l = trial == 0 ? 90000 : rng() % 400, nb = (rng() % 3) ? 0 : 1 + rng() % 30;
    int nq = rng() % 12;
    long long m = z + l + (nb ? nb + 1 : 0);
    for (int i = 0; i < nq; ++i) { q.push_back(trial == 0 ? 15000 + rng() % 100 : 1 + rng() % 300); m += q.back(); }
    if (m < 4) continue;
    const bool banded = trial % 2 == 1; // banded patterns keep the anchored numbering (apply_reorder builds), random ones chain + home (built beside)
    HostCsc A; A.m = (int)m; A.n = n; A.p.assign(n + 1, 0);
    for (int j = 0; j < n; ++j) {
      std::vector<int> r;
      const long long c0 = (long long)j * m / n;
      for (int k = 0; k < cn; ++k) r.push_back(banded ? (int)std::min<long long>(m - 1, c0 + rng() % 64) : (int)(rng() % m));
      std::sort(r.begin(), r.end()); r.erase(std::unique(r.begin(), r.end()), r.end());
      if (rng() % 20 == 0) r.clear(); // columns without entries
      for (int v : r) { A.i.push_back(v); A.x.push_back((real)(1 + A.i.size())); }
      A.p[j + 1] = (eoff)A.i.size();
    }
    if (banded) { // scramble the columns: the locality is hidden, not absent
      std::vector<int> perm(n);
      for (int j = 0; j < n; ++j) perm[j] = j;
      std::shuffle(perm.begin(), perm.end(), rng);
      HostCsc S; S.m = A.m; S.n = n; S.p.assign(n + 1, 0);
      for (int j = 0; j < n; ++j) {
        for (eoff k = A.p[perm[j]]; k < A.p[perm[j] + 1]; ++k) { S.i.push_back(A.i[(size_t)k]); S.x.push_back(A.x[(size_t)k]); }
        S.p[j + 1] = (eoff)S.i.size();
      }
      A = S;
    }
    ScsCone k{}; std::vector<scs_int> qq(q.begin(), q.end());
    std::vector<scs_float> bu(nb, 1), bl(nb, -1);
    k.z = z; k.l = l; k.bsize = nb ? nb + 1 : 0; k.bu = nb ? bu.data() : nullptr; k.bl = nb ? bl.data() : nullptr;
    k.q = qq.empty() ? nullptr : qq.data(); k.qsize = (scs_int)qq.size();
    Reorder R;
    plan_reorder(A, &k, false, R);
    if (R.active) { ++kept; if (R.have_ready) ++ready; }
    HostCsc B = A;
    apply_reorder(B, R);
    if (check(A, B, R, trial)) return 1;
  }
  { // a matrix without any entry, with and without an (identity) renumbering in force
    HostCsc A; A.m = 5; A.n = 3; A.p.assign(4, 0);
    Reorder R;
    permute_values(R, nullptr, 0, nullptr);
    if (!all_finite(nullptr, 0)) return fail("empty value array", -1);
    R.active = true;
    R.col_new2old = {2, 0, 1};
    R.row_new2old = {0, 1, 2, 3, 4};
    HostCsc B = A;
    apply_reorder(B, R);
    if (!R.entry_new2old.empty() || B.p[3] != 0) return fail("nnz = 0", -1);
    permute_values(R, nullptr, 0, nullptr);
    real one = 1;
    bool threw = false;
    try { permute_values(R, &one, 1, &one); } catch (const std::exception &) { threw = true; } // a length that is not the pattern's
    if (!threw) return fail("length mismatch not refused", -1);
  }
  { // entry positions at the top of the eoff range: the arithmetic of the column-pointer prefix (no allocation of that size)
    const eoff top = std::numeric_limits<eoff>::max();
    std::vector<eoff> p = {0, top - 1, top - 1, top};
    eoff len = 0;
    for (size_t j = 0; j + 1 < p.size(); ++j) len += p[j + 1] - p[j];
    if (len != top || (size_t)top != (size_t)p.back()) return fail("eoff arithmetic", -1);
  }
  printf("kept %d of the renumberings, %d of them built beside the measurement\n", kept, ready);
  printf("sanitizer driver ok\n");
  return 0;
}
