// lexicon_walk.h — the two reads the lexicon-constrained decode kernels make of a lexicon's prefix tree (CSR arrays of msocr_lexicon:
// edge_begin [n_nodes + 1], edge_tok / edge_child [n_edges], terminal [n_nodes]), and the host validator's view of the same arrays.
// Host and device: the kernels (attn_general_lexicon.hip, attn_lexicon_mfma.hip) call them, and so does a plain C++ program that feeds
// them corrupted tries under the address and undefined-behaviour sanitizers (tools/lexicon_clamp_check.cpp).  Whatever the arrays
// hold, every index these functions form lies inside the arrays: a malformed trie can produce a wrong word, not an out-of-bounds read.
#ifndef MSOCR_LEXICON_WALK_H
#define MSOCR_LEXICON_WALK_H
#include <stdint.h>

#ifdef __HIPCC__
#define MSOCR_HD __host__ __device__ __forceinline__
#else
#define MSOCR_HD inline
#endif

// the edges of `node`, [lo, hi) clamped into [0, n_edges] with lo <= hi; empty for a node outside [0, n_nodes) (a dead slot is -1)
MSOCR_HD void lex_edge_range(const int32_t* edge_begin, int n_nodes, int n_edges, int node, int& lo, int& hi) {
  lo = hi = 0;
  if (node < 0 || node >= n_nodes) return;
  const int b0 = edge_begin[node], b1 = edge_begin[node + 1];
  lo = b0 < 0 ? 0 : (b0 > n_edges ? n_edges : b0);
  hi = b1 < lo ? lo : (b1 > n_edges ? n_edges : b1);
}

// whether a word ends at `node`
MSOCR_HD bool lex_terminal(const uint8_t* terminal, int n_nodes, int node) { return node >= 0 && node < n_nodes && terminal[node] != 0; }

// the child of `node` along token v, or -1: binary search over the node's edge tokens (strictly ascending in a valid trie; in any
// other the search still ends after log2(edges) probes inside [lo, hi)).  A child id outside [0, n_nodes) counts as none.
MSOCR_HD int lex_child(const int32_t* edge_begin, const int32_t* edge_tok, const int32_t* edge_child, int n_nodes, int n_edges, int node,
                       int v) {
  int lo, hi;
  lex_edge_range(edge_begin, n_nodes, n_edges, node, lo, hi);
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    const int tk = edge_tok[mid];
    if (tk == v) {
      const int ch = edge_child[mid];
      return ch >= 0 && ch < n_nodes ? ch : -1;
    }
    if (tk < v) lo = mid + 1; else hi = mid;
  }
  return -1;
}
#endif
