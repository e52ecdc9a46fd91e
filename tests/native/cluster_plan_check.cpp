// Stand-alone check of build_cluster_plan and build_band_plan (phm_sched.h): what every workgroup of the cluster pruning kernels
// (phm_narrow.hip, phm_tiles.hip) reads.  Built with the host compiler and -fsanitize=address,undefined together with phm_sched.cpp
// by tests/test_narrow_classes_cpu.py, which compares the printed tier and cluster sizes with those tests/narrowclasses.py derives.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "phm_sched.h"

namespace {

struct Shape {                       // a rooted binary tree: node 0 is the root, kid0[v] = -1 for a tip
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

int fail(const std::string& name, const std::string& what) {
  std::fprintf(stderr, "%s: %s\n", name.c_str(), what.c_str());
  return 1;
}

// one plan: `max_nodes` nodes per cluster at the most; `band` > 0: the band plan's extra rules
int check_plan(const std::string& name, const phm::Schedule& s, const phm::ClusterPlan& plan, int max_nodes, int band) {
  const int Nn = s.n_node;
  const std::vector<int32_t> height = phm::node_heights(s.up);
  std::vector<int> step_of(Nn, -1);
  for (int k = 0; k < Nn; ++k) step_of[s.up[k].parent] = k;
  const int n_clusters = (int)plan.item_off.size() - 1;
  // the offset arrays tile what they point into
  if (n_clusters < 1 || plan.item_off.front() != 0 || plan.item_off.back() != (int)plan.nodes.size()) return fail(name, "item_off does not span the nodes");
  if ((int)plan.nodes.size() != Nn) return fail(name, "the plan does not hold one entry per internal node");
  if ((int)plan.lvl_ptr.size() != n_clusters + 1 || plan.lvl_ptr.front() != 0 || plan.lvl_ptr.back() != (int)plan.lvl_off.size())
    return fail(name, "lvl_ptr does not span lvl_off");
  if (plan.tier_off.size() < 2 || plan.tier_off.front() != 0 || plan.tier_off.back() != n_clusters) return fail(name, "tier_off does not span the clusters");
  for (size_t t = 0; t + 1 < plan.tier_off.size(); ++t)
    if (plan.tier_off[t + 1] <= plan.tier_off[t]) return fail(name, "an empty or reversed tier");
  std::vector<int> tier_of(n_clusters, -1);
  for (size_t t = 0; t + 1 < plan.tier_off.size(); ++t)
    for (int c = plan.tier_off[t]; c < plan.tier_off[t + 1]; ++c) tier_of[c] = (int)t;
  // every internal node in exactly one cluster
  std::vector<int> cluster_of(Nn, -1), pos_of(Nn, -1);
  for (int c = 0; c < n_clusters; ++c) {
    const int i0 = plan.item_off[c], i1 = plan.item_off[c + 1];
    if (i1 <= i0) return fail(name, "an empty or reversed cluster");
    if (i1 - i0 > max_nodes) return fail(name, "a cluster with too many nodes");
    for (int i = i0; i < i1; ++i) {
      const int v = plan.nodes[i].parent;
      if (v < 0 || v >= Nn) return fail(name, "a node outside the tree");
      if (cluster_of[v] >= 0) return fail(name, "a node twice");
      cluster_of[v] = c; pos_of[v] = i - i0;
    }
  }
  for (int v = 0; v < Nn; ++v) if (cluster_of[v] < 0) return fail(name, "a node missing");
  for (int c = 0; c < n_clusters; ++c) {
    const int i0 = plan.item_off[c], i1 = plan.item_off[c + 1];
    // height levels: lvl_off at exactly the height changes
    const int l0 = plan.lvl_ptr[c], l1 = plan.lvl_ptr[c + 1];
    if (l1 - l0 < 2 || plan.lvl_off[l0] != i0 || plan.lvl_off[l1 - 1] != i1) return fail(name, "the levels of a cluster do not span it");
    for (int l = l0; l + 1 < l1; ++l) {
      const int a = plan.lvl_off[l], b = plan.lvl_off[l + 1];
      if (b <= a) return fail(name, "an empty or reversed level");
      for (int i = a + 1; i < b; ++i)
        if (height[plan.nodes[i].parent] != height[plan.nodes[a].parent]) return fail(name, "two heights in one level");
      if (l + 2 < l1 && height[plan.nodes[b].parent] <= height[plan.nodes[a].parent]) return fail(name, "levels not in increasing height");
    }
    for (int i = i0; i < i1; ++i) {
      const phm::ClusterNode& nd = plan.nodes[i];
      const phm::UpStep& u = s.up[step_of[nd.parent]];
      for (int k = 0; k < 2; ++k) {
        if (nd.child[k] != u.child[k] || nd.edge[k] != u.edge[k]) return fail(name, "a record differs from the pruning step of its node");
        const int ch = nd.child[k];
        if (ch >= 0 && cluster_of[ch] == c) {        // a child of the same cluster: by position, lower than the node's own
          if (nd.slot[k] != pos_of[ch]) return fail(name, "slot is not the position of the child");
          if (nd.slot[k] < 0 || nd.slot[k] >= i - i0) return fail(name, "the child's position is not below the node's");
          if (plan.nodes[i0 + nd.slot[k]].parent != ch) return fail(name, "slot points at another node");
        } else {                                     // outside: a tip, or a cluster of an earlier tier
          if (nd.slot[k] != -1) return fail(name, "slot set for a child outside the cluster");
          if (ch >= 0 && tier_of[cluster_of[ch]] >= tier_of[c]) return fail(name, "a child outside the cluster that is not in an earlier tier");
        }
      }
    }
  }
  // clusters of a tier: the largest first
  for (size_t t = 0; t + 1 < plan.tier_off.size(); ++t)
    for (int c = plan.tier_off[t] + 1; c < plan.tier_off[t + 1]; ++c)
      if (plan.item_off[c + 1] - plan.item_off[c] > plan.item_off[c] - plan.item_off[c - 1]) return fail(name, "a tier not sorted by size");
  // the last tier holds the root; the band plan's last tier is that one cluster
  if (tier_of[cluster_of[s.root]] != (int)plan.tier_off.size() - 2) return fail(name, "the root is not in the last tier");
  if (band > 0) {
    if (plan.tier_off[plan.tier_off.size() - 1] - plan.tier_off[plan.tier_off.size() - 2] != 1) return fail(name, "the last band tier is not one cluster");
    for (int v = 0; v < Nn; ++v)
      if (tier_of[cluster_of[v]] != height[v] / band) return fail(name, "a node outside the band of its height");
  }
  std::printf("%s:", name.c_str());
  for (size_t t = 0; t + 1 < plan.tier_off.size(); ++t) {
    std::printf("%s", t ? " | " : " ");
    for (int c = plan.tier_off[t]; c < plan.tier_off[t + 1]; ++c)
      std::printf("%s%d", c > plan.tier_off[t] ? "," : "", plan.item_off[c + 1] - plan.item_off[c]);
  }
  std::printf("\n");
  return 0;
}

int check(const char* name, const Shape& t) {
  int T = 0;
  const std::vector<int32_t> edge = edge_table(t, T);
  const int E = 2 * T - 2, Nn = T - 1;
  phm::Schedule s;
  std::string err;
  if (!phm::build_schedule(T, Nn, E, edge.data(), s, err)) return fail(name, "build_schedule: " + err);
  phm::ClusterPlan cl, bd;
  phm::build_cluster_plan(s, 256, cl);
  phm::build_band_plan(s, 8, bd);
  return check_plan(std::string(name) + " clusters", s, cl, 256, 0) + check_plan(std::string(name) + " bands", s, bd, 255, 8);
}

Shape ladder(int tips) {             // one tip and one internal child per node
  Shape t; t.add();
  int v = 0;
  for (int k = 0; k < tips - 1; ++k) { t.split(v); v = t.kid1[v]; }
  return t;
}

void grow_balanced(Shape& t, int v, int tips, std::vector<int>& leaves) {      // ceil(tips / 2) below the first child
  if (tips == 1) { leaves.push_back(v); return; }
  t.split(v);
  const int a = t.kid0[v], b = t.kid1[v];
  grow_balanced(t, a, (tips + 1) / 2, leaves);
  grow_balanced(t, b, tips / 2, leaves);
}

Shape balanced(int tips) {
  Shape t; t.add();
  std::vector<int> leaves;
  grow_balanced(t, 0, tips, leaves);
  return t;
}

Shape cherries(int top, int k) {     // a balanced top of `top` leaves, the first k of them (left to right) made cherries
  Shape t; t.add();
  std::vector<int> leaves;
  grow_balanced(t, 0, top, leaves);
  for (int i = 0; i < k; ++i) t.split(leaves[i]);
  return t;
}

Shape random_tree(int tips) {
  Shape t; t.add();
  std::vector<int> open = {0};
  uint64_t x = 0x9e3779b97f4a7c15ull;
  while ((int)open.size() < tips) {
    x = x * 6364136223846793005ull + 1442695040888963407ull;
    const size_t i = (size_t)((x >> 33) % open.size());
    const int v = open[i];
    t.split(v);
    open[i] = t.kid0[v]; open.push_back(t.kid1[v]);
  }
  return t;
}

}  // namespace

int main() {
  int bad = 0;
  bad += check("ladder 2", ladder(2));
  for (int tips : {257, 258, 700}) bad += check(("ladder " + std::to_string(tips)).c_str(), ladder(tips));
  for (int tips : {256, 257, 258, 1024}) bad += check(("balanced " + std::to_string(tips)).c_str(), balanced(tips));
  bad += check("random 1000", random_tree(1000));
  const int cherry[][2] = {{64, 63}, {64, 64}, {65, 65}, {128, 65}, {128, 128}, {1024, 1024}, {2048, 1025}};
  for (const auto& c : cherry) bad += check(("cherries " + std::to_string(c[0]) + " " + std::to_string(c[1])).c_str(), cherries(c[0], c[1]));
  if (bad) return 1;
  std::printf("ok\n");
  return 0;
}
