// What the three sources of the host model share (internal): cmx_host_tree.cpp (tree, walk program), cmx_host_verify.cpp
// (numeric self-check) and cmx_host_model.cpp (substitution model, device layouts, build_host_model).
#pragma once
#include "cmx_host_model.h"
#include "cmx_walk.h"

namespace cmx {

// Backend::rec of the host backends: record v of the walk
inline void copy_record(const HostModel& hm, int v, int (&r)[16]) { for (int i = 0; i < 16; ++i) r[i] = hm.nrec[(size_t)v * 16 + i]; }

inline std::vector<int> children(const HostModel& hm, int n) {
  std::vector<int> v;
  for (int e = hm.first_child[n]; e >= 0; e = hm.next_sib[e]) v.push_back(e);
  return v;
}

// the members of the backend concept that apply no operator and move no workspace vector: nothing to list for them
struct RegisterOpsIgnored {
  template <int D, int S> void mov() {}
  template <int D, int S> void mul() {}
  template <int D, int A, int B> void prod() {}
  void mulup() {}
  template <int D> void setpi() {}
  template <int S> void rootl() {}
  void dot3(int) {}
  template <int R> void kill() {}
};

// Stages of build_host_model (cmx_host_tree.cpp).  build_tree: the tree's checks in their order, then parent -> first_child /
// next_sib / taxon_of / slot / int_post; error message or empty string.  The other two cannot fail.
std::string build_tree(const cmx_tree* tree, HostModel* hm);
void build_walk_program(HostModel* hm);   // fuse, records, LDS-slot plan, cherry numbering, streams (nothing on the plain path)
void build_sim_groups(HostModel* hm);     // simg, simord

}  // namespace cmx
