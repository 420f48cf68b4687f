// dev: the defensive clamps of csrc/lexicon_walk.h on the host.  The constrained decode kernels read a lexicon's prefix tree through
// lex_edge_range / lex_terminal / lex_child alone; this program runs the kernels' two uses of them (the edge walk that builds the
// allowed-token mask, and the child lookup of the bookkeeping) over a valid trie and over corrupted copies of it, every array in a heap
// block of its exact size, so that the address sanitizer sees any index outside the arrays and the undefined-behaviour sanitizer any
// overflow.  Build and run (CPU only):
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Imanuscript_ocr_amd/csrc tools/lexicon_clamp_check.cpp \
//       -o /tmp/lexicon_clamp_check && /tmp/lexicon_clamp_check
// Prints the number of tries and probes and "OK"; a sanitizer report (and a non-zero exit) is a failure.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <random>
#include <vector>

#include "lexicon_walk.h"

struct Trie {  // exact-size heap blocks
  int32_t *begin, *tok, *child;
  uint8_t* term;
  int n_nodes, n_edges;
};

static Trie make(const std::vector<int32_t>& b, const std::vector<int32_t>& t, const std::vector<int32_t>& c, const std::vector<uint8_t>& z) {
  Trie r;
  r.n_nodes = (int)z.size();
  r.n_edges = (int)t.size();
  r.begin = (int32_t*)malloc(b.size() * 4); memcpy(r.begin, b.data(), b.size() * 4);
  r.tok = (int32_t*)malloc(t.size() * 4 + 0); if (!t.empty()) memcpy(r.tok, t.data(), t.size() * 4);
  r.child = (int32_t*)malloc(c.size() * 4 + 0); if (!c.empty()) memcpy(r.child, c.data(), c.size() * 4);
  r.term = (uint8_t*)malloc(z.size()); memcpy(r.term, z.data(), z.size());
  return r;
}
static void drop(Trie& r) { free(r.begin); free(r.tok); free(r.child); free(r.term); }

// what a decode step does with one slot: the mask walk, then the child lookup for every token (and a few outside [0, V))
static long probe(const Trie& r, int V, int node, unsigned* mask) {
  long n = 0;
  int lo, hi;
  lex_edge_range(r.begin, r.n_nodes, r.n_edges, node, lo, hi);
  if (lo < 0 || hi > r.n_edges || lo > hi) { printf("range outside [0, n_edges]\n"); exit(1); }
  for (int e = lo; e < hi; ++e) {
    const int tk = r.tok[e];
    if (tk >= 0 && tk < V) mask[tk >> 5] |= 1u << (tk & 31);
  }
  n += lex_terminal(r.term, r.n_nodes, node);
  for (int v = -2; v < V + 2; ++v) {
    const int ch = lex_child(r.begin, r.tok, r.child, r.n_nodes, r.n_edges, node, v);
    if (ch < -1 || ch >= r.n_nodes) { printf("child outside [-1, n_nodes)\n"); exit(1); }
    ++n;
  }
  return n;
}

int main() {
  const int V = 70;
  std::mt19937 rng(7);
  // a valid trie over random words, breadth-first: built level by level
  std::vector<std::vector<int>> words;
  for (int i = 0; i < 300; ++i) {
    std::vector<int> w(1 + rng() % 8);
    for (auto& t : w) t = 4 + rng() % 12;
    words.push_back(w);
  }
  std::vector<std::vector<std::pair<int, int>>> kids(1);  // node -> sorted (tok, child) in insertion trie
  std::vector<uint8_t> term0(1, 0);
  for (auto& w : words) {
    int n = 0;
    for (int t : w) {
      int m = -1;
      for (auto& e : kids[n]) if (e.first == t) m = e.second;
      if (m < 0) { m = (int)kids.size(); kids[n].push_back({t, m}); kids.emplace_back(); term0.push_back(0); }
      n = m;
    }
    term0[n] = 1;
  }
  std::vector<int> order(1, 0);
  std::vector<int32_t> b(1, 0), t, c;
  std::vector<uint8_t> z;
  for (size_t i = 0; i < order.size(); ++i) {
    auto es = kids[order[i]];
    for (size_t x = 0; x < es.size(); ++x)
      for (size_t y = x + 1; y < es.size(); ++y)
        if (es[y].first < es[x].first) std::swap(es[x], es[y]);
    for (auto& e : es) { t.push_back(e.first); c.push_back((int32_t)order.size()); order.push_back(e.second); }
    b.push_back((int32_t)t.size());
    z.push_back(term0[order[i]]);
  }
  long probes = 0, tries = 0;
  unsigned mask[16];
  const int32_t bad[] = {INT32_MIN, -1000000, -1, 0, 1, 69, 70, 1000000, INT32_MAX};
  for (int round = 0; round < 400; ++round) {
    std::vector<int32_t> b2 = b, t2 = t, c2 = c;
    std::vector<uint8_t> z2 = z;
    if (round) {  // round 0: the valid trie; then 1..6 corruptions per copy, over all three index arrays
      for (int k = 0, nk = 1 + rng() % 6; k < nk; ++k) {
        const int32_t val = (rng() % 3) ? bad[rng() % 9] : (int32_t)rng();
        switch (rng() % 4) {
          case 0: b2[rng() % b2.size()] = val; break;
          case 1: t2[rng() % t2.size()] = val; break;
          case 2: c2[rng() % c2.size()] = val; break;
          default: z2[rng() % z2.size()] ^= 1; break;
        }
      }
      if (round % 7 == 0) std::shuffle(t2.begin(), t2.end(), rng);  // unsorted tokens everywhere
    }
    Trie r = make(b2, t2, c2, z2);
    // a slot's walk along its own children, as the decode does, from the root and from arbitrary node ids (the kernels only ever
    // hold -1 or a node lex_child returned, i.e. inside [0, n_nodes); ids outside are probed all the same)
    for (int node = -2; node < r.n_nodes + 2; ++node) { memset(mask, 0, sizeof mask); probes += probe(r, V, node, mask); }
    probes += probe(r, V, INT32_MAX, mask) + probe(r, V, INT32_MIN, mask);
    // the struct's sizes lying low is allowed too (a caller may pass fewer nodes / edges than the arrays hold)
    Trie small = r; small.n_nodes = r.n_nodes / 2; small.n_edges = r.n_edges / 3;
    for (int node = -1; node < small.n_nodes + 1; ++node) { memset(mask, 0, sizeof mask); probes += probe(small, V, node, mask); }
    drop(r);
    ++tries;
  }
  printf("%ld tries (%d nodes, %d edges each), %ld lookups: OK\n", tries, (int)z.size(), (int)t.size(), probes);
  return 0;
}
