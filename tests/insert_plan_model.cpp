// CPU model of the window-parallel insert phase (fqsx_dev.h: insert_windows) against the one-key-at-a-time insert.
// Built and run by tests/test_insert_plan.py with -fsanitize=address,undefined; includes the draw rule the kernel uses
// (fqsx_insplan.h) as it stands.  The table is a plain array of counters indexed by the key (0: absent).
#include "fqsx_insplan.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

typedef uint32_t u32;
struct Cinc { u32 thr, mult, maxv, cm; };

static u32 n_draws_ref, n_draws_win, n_par, n_in_order, n_ambiguous;

// insert(), ht_kmer.h:420-438 with the CCounterIncrementer of utils.h:256-335 -- what insert_batch_k reproduces
static void insert_one(std::vector<u32> &tab, u32 key, const Cinc &c, std::mt19937 &rng, u32 &draws) {
  const u32 cnt = tab[key];
  if (cnt == 0) { tab[key] = 1; return; }
  if (cnt <= c.thr) { if (cnt < c.cm) tab[key] = cnt + 1; return; }
  if (cnt < c.maxv) {
    ++draws;
    if (rng() % (c.mult * (cnt - c.thr)) == 0) tab[key] = cnt + 1;
  }
}

// one window, the kernel's stages in the kernel's order; returns false when the window had to go in order
static bool insert_window(std::vector<u32> &tab, const u32 *keys, u32 n, const Cinc &c, u32 maxmult, std::mt19937 &rng, u32 &draws) {
  std::vector<u32> c0(n), rank(n), dnum(n);
  std::vector<char> drw(n);
  // locate (read-only)
  for (u32 i = 0; i < n; ++i) c0[i] = tab[keys[i]];
  // rank: rounds over the keys still unranked, the smallest index of every k-mer wins the round
  std::vector<u32> best(tab.size());
  std::vector<char> ranked(n, 0);
  u32 q = 0;
  bool over = false;
  for (;;) {
    std::fill(best.begin(), best.end(), ~0u);
    for (u32 i = 0; i < n; ++i) if (!ranked[i]) best[keys[i]] = std::min(best[keys[i]], i);
    bool left = false;
    for (u32 i = 0; i < n; ++i) if (!ranked[i]) { if (best[keys[i]] == i) { rank[i] = q; ranked[i] = 1; } else left = true; }
    if (!left) break;
    if (++q >= maxmult) { over = true; break; }
  }
  // decide, before anything is written
  bool amb = over;
  for (u32 i = 0; i < n && !amb; ++i) amb = insplan_ambiguous(c0[i], rank[i], c.thr, c.maxv);
  if (amb) {
    if (!over) ++n_ambiguous;
    for (u32 i = 0; i < n; ++i) insert_one(tab, keys[i], c, rng, draws);
    return false;
  }
  // draw numbers: exclusive scan of the flags in index order, then that many outputs of the stream
  u32 D = 0;
  for (u32 i = 0; i < n; ++i) { drw[i] = insplan_draws(c0[i], rank[i], c.thr, c.maxv); dnum[i] = D; D += drw[i] ? 1u : 0u; }
  std::vector<u32> rnd(D);
  for (u32 d = 0; d < D; ++d) rnd[d] = rng();
  draws += D;
  // claim
  for (u32 i = 0; i < n; ++i) if (c0[i] == 0 && rank[i] == 0) tab[keys[i]] = 1;
  // commit in rank rounds (inside a round the keys are all different: any order)
  for (u32 r = 0; r <= q; ++r)
    for (u32 ii = n; ii-- > 0;) {
      const u32 i = ii;
      if (rank[i] != r || (c0[i] == 0 && r == 0)) continue;
      const u32 cnt = r == 0 ? c0[i] : tab[keys[i]];
      if (insplan_adds(cnt, drw[i] != 0, drw[i] ? rnd[dnum[i]] : 0u, c.thr, c.mult, c.cm)) tab[keys[i]] = cnt + 1;
    }
  return true;
}

static int run_case(u32 alphabet, u32 win, const Cinc &c, u32 maxmult, u32 seed, bool preload) {
  const u32 N = 5000;
  std::mt19937 gen(seed);
  std::vector<u32> keys(N);
  for (u32 i = 0; i < N; ++i) {   // heavy duplication; a quarter of the keys come from the first eighth of the alphabet
    const u32 a = gen() % 4 == 0 ? std::max(1u, alphabet / 8) : alphabet;
    keys[i] = gen() % a;
  }
  std::vector<u32> ref(alphabet, 0), par(alphabet, 0);
  if (preload)   // counters around the threshold and below the maximum, as a table has them late in a file
    for (u32 k = 0; k < alphabet; ++k) {
      const u32 r = (u32)gen() % 4, x = (u32)gen();
      ref[k] = par[k] = r == 0 ? 0 : r == 1 ? c.thr - std::min(c.thr, x % 3) : r == 2 ? c.thr + 1 + x % (c.maxv - c.thr) : c.maxv - std::min(c.maxv - 1, x % 40);
    }
  std::mt19937 rng_ref(5481), rng_par(5481);
  u32 d_ref = 0, d_par = 0;
  for (u32 o = 0; o < N; o += win) {
    const u32 n = std::min(win, N - o);
    for (u32 i = 0; i < n; ++i) insert_one(ref, keys[o + i], c, rng_ref, d_ref);
    if (insert_window(par, keys.data() + o, n, c, maxmult, rng_par, d_par)) ++n_par; else ++n_in_order;
    if (ref != par || !(rng_ref == rng_par) || d_ref != d_par) {
      fprintf(stderr, "MISMATCH alphabet %u window %u thr %u maxv %u preload %d at key %u: counters %s, stream %s, draws %u / %u\n", alphabet, win,
              c.thr, c.maxv, (int)preload, o, ref == par ? "equal" : "differ", rng_ref == rng_par ? "equal" : "differs", d_ref, d_par);
      return 1;
    }
  }
  n_draws_ref += d_ref; n_draws_win += d_par;
  return 0;
}

int main() {
  const Cinc kinds[3] = {{7, 2, 63, 63}, {2047, 1, 4095, 4095}, {1, 1, 4, 7}};   // b-mers, s-mers, and a tiny pair that saturates inside a window
  const u32 alphabets[4] = {8, 37, 200, 1}, windows[4] = {1, 7, 64, 2048};
  int bad = 0;
  u32 seed = 1;
  for (const Cinc &c : kinds)
    for (u32 a : alphabets)
      for (u32 w : windows)
        for (int preload = 0; preload < 2; ++preload) {
          bad += run_case(a, w, c, 16, seed++, preload != 0);
          bad += run_case(a, w, c, 1, seed++, preload != 0);
        }
  printf("cases %u windows_parallel %u windows_in_order %u (ambiguous %u) draws %u\n", seed - 1, n_par, n_in_order, n_ambiguous, n_draws_win);
  if (bad) return 1;
  if (n_in_order == 0 || n_ambiguous == 0 || n_par == 0 || n_draws_win == 0 || n_draws_ref != n_draws_win) { fprintf(stderr, "the cases do not reach both paths\n"); return 2; }
  return 0;
}
