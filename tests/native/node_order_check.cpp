// Stand-alone check of node_depth_levels (phm_sched.h): the order of the node draws of phm_tiles.hip, an item per internal node.
// Built with the host compiler and -fsanitize=address,undefined together with phm_sched.cpp by tests/test_node_order_cpu.py.
#include <cstdint>
#include <cstdio>
#include <functional>
#include <string>
#include <vector>

#include "phm_sched.h"

namespace {

struct Shape {                       // a rooted binary tree: node 0 is the root, kids[v] = {-1, -1} for a tip
  std::vector<int> kid0, kid1;
  int add() { kid0.push_back(-1); kid1.push_back(-1); return (int)kid0.size() - 1; }
  void split(int v) { const int a = add(), b = add(); kid0[v] = a; kid1[v] = b; }
};

// edge table as R's ape writes it: tips 1 .. T, root T + 1, rows in cladewise order; column-major n_edge x 2
std::vector<int32_t> edge_table(const Shape& t, int& n_tips) {
  const int n = (int)t.kid0.size();
  n_tips = (n + 1) / 2;
  std::vector<int> id(n, 0);
  int next_tip = 1, next_int = n_tips + 1;
  std::vector<int> stack = {0};
  std::vector<int> order;
  while (!stack.empty()) {           // pre-order, first child first
    const int v = stack.back(); stack.pop_back();
    order.push_back(v);
    id[v] = t.kid0[v] < 0 ? next_tip++ : next_int++;
    if (t.kid0[v] >= 0) { stack.push_back(t.kid1[v]); stack.push_back(t.kid0[v]); }
  }
  std::vector<int> parent(n, -1);
  for (int v = 0; v < n; ++v) if (t.kid0[v] >= 0) { parent[t.kid0[v]] = v; parent[t.kid1[v]] = v; }
  const int E = n - 1;
  std::vector<int32_t> edge(2 * (size_t)E);
  int r = 0;
  for (int v : order) if (parent[v] >= 0) { edge[r] = id[parent[v]]; edge[E + r] = id[v]; ++r; }
  return edge;
}

int fail(const char* name, const std::string& what) {
  std::fprintf(stderr, "%s: %s\n", name, what.c_str());
  return 1;
}

int check(const char* name, const Shape& t) {
  int T = 0;
  const std::vector<int32_t> edge = edge_table(t, T);
  const int E = 2 * T - 2, Nn = T - 1;
  phm::Schedule s;
  std::string err;
  if (!phm::build_schedule(T, Nn, E, edge.data(), s, err)) return fail(name, "build_schedule: " + err);
  std::vector<int32_t> order, off, eorder, eoff;
  phm::node_depth_levels(s, order, off);
  phm::depth_levels(s, eorder, eoff);
  if ((int)order.size() != Nn) return fail(name, "the order does not hold one entry per internal node");
  // the level offsets tile the order, no level is empty, and the levels number those of the edge order (two edges per node)
  if (off.empty() || off.front() != 0 || off.back() != Nn) return fail(name, "the level offsets do not span the order");
  if (off.size() != eoff.size()) return fail(name, "node levels and edge levels differ in number");
  for (size_t l = 0; l + 1 < off.size(); ++l) {
    if (off[l + 1] <= off[l]) return fail(name, "an empty or reversed level");
    if (eoff[l + 1] - eoff[l] != 2 * (off[l + 1] - off[l])) return fail(name, "a level does not hold two edges per node");
  }
  // every internal node exactly once
  std::vector<int> level_of(Nn, -1);
  for (size_t l = 0; l + 1 < off.size(); ++l)
    for (int i = off[l]; i < off[l + 1]; ++i) {
      const int k = order[i];
      if (k < 0 || k >= Nn) return fail(name, "a position outside the pruning steps");
      const int node = s.up[k].parent;
      if (node < 0 || node >= Nn || level_of[node] >= 0) return fail(name, "a node twice");
      level_of[node] = (int)l;
    }
  for (int v = 0; v < Nn; ++v) if (level_of[v] < 0) return fail(name, "a node missing");
  // the root alone at level 0; a node's parent one level earlier
  if (level_of[s.root] != 0 || off[1] != 1) return fail(name, "level 0 is not the root alone");
  for (const phm::UpStep& u : s.up)
    for (int c = 0; c < 2; ++c)
      if (u.child[c] >= 0 && level_of[u.child[c]] != level_of[u.parent] + 1) return fail(name, "a child not one level below its parent");
  // stable inside a level
  for (size_t l = 0; l + 1 < off.size(); ++l)
    for (int i = off[l] + 1; i < off[l + 1]; ++i)
      if (order[i - 1] >= order[i]) return fail(name, "a level is not in the order of the pruning steps");
  std::printf("%s: %d nodes in %d levels\n", name, Nn, (int)off.size() - 1);
  return 0;
}

}  // namespace

int main() {
  int bad = 0;
  {
    Shape t; t.add(); t.split(0);
    bad += check("two tips", t);
  }
  {
    Shape t; t.add(); t.split(0);
    bad += check("three tips", (t.split(2), t));
  }
  {
    Shape t; t.add();
    int v = 0;
    for (int k = 0; k < 299; ++k) { t.split(v); v = t.kid1[v]; }      // a ladder: one tip and one internal child per node
    bad += check("ladder", t);
  }
  {
    Shape t; t.add();
    std::vector<int> tips = {0};
    for (int d = 0; d < 6; ++d) {
      std::vector<int> next;
      for (int v : tips) { t.split(v); next.push_back(t.kid0[v]); next.push_back(t.kid1[v]); }
      tips.swap(next);
    }
    bad += check("balanced", t);
  }
  {
    Shape t; t.add();
    std::vector<int> tips = {0};
    uint64_t x = 0x9e3779b97f4a7c15ull;
    while ((int)tips.size() < 1000) {
      x = x * 6364136223846793005ull + 1442695040888963407ull;
      const size_t i = (size_t)((x >> 33) % tips.size());
      const int v = tips[i];
      t.split(v);
      tips[i] = t.kid0[v]; tips.push_back(t.kid1[v]);
    }
    bad += check("random 1000", t);
  }
  if (bad) return 1;
  std::printf("ok\n");
  return 0;
}
