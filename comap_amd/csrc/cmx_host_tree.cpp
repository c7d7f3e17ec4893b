// Host model, the tree (see cmx_host_model.h): validation and topology, the simulator's level groups, and the program the
// mapping wave follows.  Plain C++17, no device code.
#include "cmx_host_parts.h"

#include <algorithm>
#include <array>
#include <atomic>
#include <cmath>

namespace cmx {

// ------------------------------------------------------------------------------------------------ tree
std::string build_tree(const cmx_tree* tree, HostModel* hm) {
  const int nn = tree->nnodes, T = tree->ntaxa;
  if (nn < 3 || T < 2 || !tree->parent || !tree->blen || !tree->leaf_of_taxon) return "tree is incomplete";
  if (nn > 65535) return "tree too large";
  hm->nn = nn; hm->B = nn - 1; hm->T = T; hm->root = nn - 1;
  hm->parent.assign(tree->parent, tree->parent + nn);
  hm->blen.assign(tree->blen, tree->blen + nn);
  // ---- tree checks: post-order, root last
  if (hm->parent[nn - 1] != -1) return "parent[root] must be -1 with the root last";
  for (int i = 0; i < nn - 1; ++i) {
    if (hm->parent[i] <= i || hm->parent[i] >= nn) return "nodes must be in post-order (parent id > child id)";
    if (!(hm->blen[i] >= 0.0) || !std::isfinite(hm->blen[i])) return "branch lengths must be finite and >= 0";
  }
  hm->first_child.assign(nn, -1);
  hm->next_sib.assign(nn, -1);
  std::vector<int> last(nn, -1), nchild(nn, 0);
  for (int i = 0; i < nn - 1; ++i) {
    const int p = hm->parent[i];
    if (hm->first_child[p] < 0) hm->first_child[p] = i; else hm->next_sib[last[p]] = i;
    last[p] = i;
    nchild[p]++;
  }
  hm->taxon_of.assign(nn, -1);
  for (int t = 0; t < T; ++t) {
    const int n = tree->leaf_of_taxon[t];
    if (n < 0 || n >= nn || nchild[n] != 0) return "leaf_of_taxon must name leaves";
    if (hm->taxon_of[n] >= 0) return "leaf_of_taxon has duplicates";
    hm->taxon_of[n] = t;
  }
  hm->slot.assign(nn, -1);
  hm->int_post.clear();
  for (int i = 0; i < nn; ++i) {
    if (nchild[i] == 0) {
      if (hm->taxon_of[i] < 0) return "every leaf needs an alignment row";
    } else {
      if (nchild[i] < 2 && i != nn - 1) return "internal nodes need at least two children";
      hm->slot[i] = (int)hm->int_post.size();
      hm->int_post.push_back(i);
    }
  }
  if (nchild[nn - 1] < 2) return "the root needs at least two children";
  hm->NI = (int)hm->int_post.size();
  return std::string();
}

// simulator: nodes by depth, four of a level at a time (a level's draws only need the level above); a short group is
// padded by repeating its last node (drawing a node twice gives the same state twice)
void build_sim_groups(HostModel* hm) {
  const int nn = hm->nn;
  std::vector<int> depth(nn, 0);
  int maxd = 0;
  for (int i = nn - 2; i >= 0; --i) { depth[i] = depth[hm->parent[i]] + 1; maxd = std::max(maxd, depth[i]); }
  std::vector<std::vector<int>> level(maxd + 1);
  for (int i = nn - 2; i >= 0; --i) level[depth[i]].push_back(i);
  hm->simg.clear();
  hm->simord.clear();
  for (int d = 1; d <= maxd; ++d) hm->simord.insert(hm->simord.end(), level[d].begin(), level[d].end());
  for (int d = 1; d <= maxd; ++d)
    for (size_t i = 0; i < level[d].size(); i += 4) {
      int g[16];
      for (int j = 0; j < 4; ++j) {
        const int n = level[d][std::min(i + j, level[d].size() - 1)];
        g[j] = n; g[4 + j] = hm->parent[n]; g[8 + j] = hm->taxon_of[n]; g[12 + j] = 0;
      }
      hm->simg.insert(hm->simg.end(), g, g + 16);
    }
}

// ------------------------------------------------------------------------------------------------ tree program
// The walk of a rate-class pass is written once (cmx_walk.h).  Here: the per-node records it reads and the Recorder
// backend that lists its operators and workspace loads in program order (what the device follows).  The Numeric backend
// that checks the whole thing before a context is accepted is in cmx_host_verify.cpp.
void build_records(HostModel* hm) {
  const int root = hm->root, nn = hm->nn;
  // ---- binary device tree: nodes 0 .. nn-1 are the tree's own, nn .. are pseudo nodes (zero-length branches) that
  // split a node with k > 2 children c1 .. ck into ((..((c1, c2), c3) ..), ck)
  std::vector<std::array<int, 2>> ch(nn, {-1, -1});
  for (int n = 0; n < nn; ++n) {
    if (hm->taxon_of[n] >= 0) continue;
    const std::vector<int> c = children(*hm, n);
    int left = c[0];
    for (size_t i = 1; i + 1 < c.size(); ++i) {
      ch.push_back({left, c[i]});
      left = (int)ch.size() - 1;
    }
    ch[n] = {left, c.back()};
  }
  const int nd = (int)ch.size();
  auto is_leaf = [&](int n) { return n < nn && hm->taxon_of[n] >= 0; };
  auto pseudo = [&](int n) { return n >= nn; };
  // workspace slots: the tree's internal nodes keep their operator slot, pseudo nodes follow
  std::vector<int> wslot(nd, -1);
  for (int n = 0; n < nn; ++n) wslot[n] = hm->slot[n];
  for (int n = nn; n < nd; ++n) wslot[n] = hm->NI + (n - nn);
  hm->NIW = hm->NI + (nd - nn);
  // inlined cherries: a (real, non-root) internal node with two leaf children is never visited
  std::vector<char> inlined(nd, 0);
  for (int n = 0; n < nn; ++n)
    if (!is_leaf(n) && n != root && is_leaf(ch[n][0]) && is_leaf(ch[n][1])) inlined[n] = 1;
  hm->cherry_of.assign(nn, -1);
  hm->ncherry = 0;
  for (int n = 0; n < nn; ++n)
    if (inlined[n]) hm->cherry_of[n] = hm->ncherry++;
  auto kind = [&](int e) { return is_leaf(e) ? (int)KIND_LEAF : (inlined[e] ? (int)KIND_CHERRY : (int)KIND_STORED); };
  // post-order of the visited nodes (explicit stack: caterpillar trees are deep)
  std::vector<int> visited, parent_d(nd, -1);
  {
    std::vector<std::pair<int, int>> st;
    st.push_back({root, 0});
    while (!st.empty()) {
      auto& top = st.back();
      const int n = top.first;
      if (is_leaf(n) || inlined[n]) { st.pop_back(); continue; }
      if (top.second < 2) {
        const int e = ch[n][top.second++];
        parent_d[e] = n;
        st.push_back({e, 0});
      } else {
        visited.push_back(n);
        st.pop_back();
      }
    }
  }
  const int NV = (int)visited.size();
  hm->NV = NV;
  hm->nrec.assign((size_t)NV * 16, -1);
  auto fill_child = [&](int* d, int e) {
    d[CH_KIND] = kind(e); d[CH_NODE] = pseudo(e) ? -1 : e; d[CH_SLOT] = is_leaf(e) ? -1 : wslot[e];
    d[CH_L1] = d[CH_L2] = -1;
    if (kind(e) == KIND_CHERRY) { d[CH_L1] = ch[e][0]; d[CH_L2] = ch[e][1]; }
  };
  for (int v = 0; v < NV; ++v) {
    const int n = visited[v];
    int* r = &hm->nrec[(size_t)v * 16];
    r[REC_NODE] = pseudo(n) ? -1 : n; r[REC_SLOT] = wslot[n]; r[2] = 2; r[REC_FLAGS] = 0;
    if (n == root) r[REC_FLAGS] |= FLAG_ROOT;
    if (pseudo(n)) r[REC_FLAGS] |= FLAG_PSEUDO;
    // the child visited right before n (inside pass) = right after n (outside pass): its vectors stay in registers
    int a = ch[n][0], b = ch[n][1];
    if (v > 0 && parent_d[visited[v - 1]] == n) {
      if (visited[v - 1] == a) std::swap(a, b);
      r[REC_FLAGS] |= FLAG_HAND;
    }
    if (v + 1 < NV && parent_d[n] == visited[v + 1]) r[REC_FLAGS] |= FLAG_U_HANDED;
    fill_child(r + REC_A, a);
    fill_child(r + REC_B, b);
  }
}

namespace {
// ---- Recorder: the operator stream (matrix index in a class block, taxon or -1) and the workspace loads of a pass.
// CM: the resolved protein walk with the cherry message table (cmx_walk.h, kCherryMsg) -- its own stream (msched_m) and
// counts (HostModel::msg); a gather adds nothing to the stream and no counted event to the wait plan.
template <bool CT, bool CR, bool CM = false>
struct Recorder : RegisterOpsIgnored {
  static constexpr bool kCherryTables = CT, kCherryRows = CR, kCherryMsg = CM;
  static constexpr bool kLdsSlot = !CT;   // the plain walk follows the plan's flags; the cherry-table walk has none (fused models)
  static_assert(!(CT && CM), "one kind of cherry table per walk");
  HostModel* hm;
  const ClassBlock blk;
  long t = 0;
  std::vector<long> store_time[2];
  struct Ld { int arr, slot; long t, src; };
  std::vector<Ld> loads;
  // what the wait plan counts (plan_waits): the pass's ops by stream index and, as -1, every workspace vector that moves
  // through HBM -- the counted walk's bookkeeping on the device (CountedWalk::load / store: vs += kVecInstrs), nothing for LDS-slot transfers
  std::vector<int> vm_events;
  explicit Recorder(HostModel* h) : hm(h), blk(h->block()) { store_time[0].assign(h->NIW, -1); store_time[1].assign(h->NIW, -1); }
  std::vector<int>& stream() { return CM ? hm->msched_m : (CT ? hm->msched_r : hm->msched); }
  void op(int mat, int tx) {
    std::vector<int>& ms = stream();
    vm_events.push_back((int)(ms.size() / 2));
    ms.push_back(mat); ms.push_back(tx); ++t;
  }
  void leaf_use(int leaf, int which) {
    const int tx = hm->taxon_of[leaf];
    op(blk.leaf(tx, which), tx);
    (CM ? hm->msg.leaf_ops : (CT ? hm->n_leaf_ops_r : hm->n_leaf_ops))++;
  }
  // cherry-table ops: the table's matrix index, both taxa in the stream entry; counted with the leaf ops
  void cherry_use(int node, int l1, int l2, int table) {
    op(blk.cherry(hm->cherry_of[node], table), cherry_entry(hm->taxon_of[l1], hm->taxon_of[l2]));
    (CT ? hm->n_leaf_ops_r : hm->n_leaf_ops)++;
  }
  void rec(int v, int (&r)[16]) const { copy_record(*hm, v, r); }
  template <int D> void lset(int leaf, int which) { leaf_use(leaf, which); }
  template <int S, int D> void lmul(int leaf, int which) { leaf_use(leaf, which); }
  template <int S> void ldot(int leaf, int which, int) { leaf_use(leaf, which); }
  template <int D> void cset(int node, int l1, int l2) {
    if constexpr (CM) { ++t; hm->msg.gathers++; }
    else cherry_use(node, l1, l2, 0);
  }
  template <int S> void cdot(int node, int l1, int l2, int table, int) { cherry_use(node, l1, l2, table); }
  template <int S, int D, bool TR> void mv(int node, int which) {
    op(blk.internal(hm->slot[node], which), -1);
    (CM ? hm->msg.products : (CT ? hm->n_products_r : hm->n_products))++;
  }
  void note_load(int arr, int slot) {
    loads.push_back({arr, slot, t++, store_time[arr][slot]});
    if (CM) hm->msg.loads++; else if (!CT) hm->n_loads++;
  }
  void note_store(int arr, int slot) {
    store_time[arr][slot] = t++;
    if (CM) hm->msg.stores++; else if (!CT) hm->n_stores++;
  }
  template <int D> void load(int arr, int slot) { note_load(arr, slot); vm_events.push_back(-1); }
  template <int S> void store(int arr, int slot) { note_store(arr, slot); vm_events.push_back(-1); }
  // transfers the LDS slot serves: still loads and stores of the walk (n_loads, n_stores, ldsched), counted beside them
  template <int D> void lload(int arr, int slot) { note_load(arr, slot); (CM ? hm->msg.lds_loads : hm->n_lds_loads)++; }
  template <int S> void lstore(int arr, int slot) { note_store(arr, slot); (CM ? hm->msg.lds_stores : hm->n_lds_stores)++; }
  template <int S> void lcopy(int, int) { ++t; (CM ? hm->msg.lds_copies : hm->n_lds_copies)++; }
};

std::atomic<int> g_wait_skew{-1};   // wait_plan_skew

// The wait plan (cmx_layout.h) of the 64-site protein walk, from the events of one recorded pass.  The count is the
// device's run-time one (cmx_map.hip: CountedState::vs / cur_seq in the kernels that keep it), replayed over two site blocks of
// all classes: a leaf op requests the next op's operator before it waits, a product after; the symbols of the next op come
// with its operator unless it is op 0 of the next site block.  An op's instances differ only there (the last op of a pass),
// and the smallest distance is kept: a smaller immediate only waits for more.  Op 0 of a block's first pass finds its
// operator behind the block prologue's drain and is served by any immediate.  Uncounted VMEM -- the epilogue between two
// blocks, compiler spills -- only adds instructions in flight behind the one waited for.
// resolved: the plan of the walk with the cherry message table, over its own stream (a gather is not an event: its loads are
// uncounted VMEM).
void plan_waits(HostModel* hm, const std::vector<int>& events, bool resolved = false) {
  const std::vector<int>& ms = resolved ? hm->msched_m : hm->msched;
  std::vector<int>& wait_dist = resolved ? hm->wait_dist_m : hm->wait_dist;
  std::vector<int>& wait_imm = resolved ? hm->wait_imm_m : hm->wait_imm;
  wait_dist.clear();
  wait_imm.clear();
  if (hm->S != 20 || hm->fuse != 1) return;
  const int n = (int)(ms.size() / 2), C = hm->C;   // (unfused: the device's classes are the model's)
  auto leaf = [&](int i) { return ms[2 * (size_t)i + 1] >= 0; };
  std::vector<long> dist(n, -1);
  long vs = kPlanRows, cur = vs;   // the kernel's first request: op 0
  for (int block = 0; block < 2; ++block)
    for (int c = 0; c < C; ++c)
      for (const int e : events) {
        if (e < 0) { vs += kPlanVec; continue; }
        const bool more = e + 1 < n;
        const int next = more ? e + 1 : 0;
        const long issued = kPlanRows + ((leaf(next) && (more || c + 1 < C)) ? 1 : 0);
        const long d = vs - cur + (leaf(e) ? issued : 0);
        // (the wave's very first op has nothing of a pass in front of it, and the prologue's drain serves it anyway)
        if (!(block == 0 && c == 0 && e == 0) && (dist[e] < 0 || d < dist[e])) dist[e] = d;
        vs += issued;
        cur = vs;
      }
  for (int i = 0; i < n; ++i) {
    wait_dist.push_back((int)dist[i]);
    wait_imm.push_back(planned_wait_imm((int)dist[i]));
  }
  // the hook names an entry of one of the two plans; the plan it names spends it
  const int held = g_wait_skew.load();
  if (held >= 0 && (held >= kWaitSkewResolved) == resolved) {
    const int skew = g_wait_skew.exchange(-1) - (resolved ? kWaitSkewResolved : 0);
    if (skew >= 0 && skew < n) wait_imm[skew] += 1;
  }
}

// the plain stream and the load schedule: the row-reusing cherry visit (cmx_walk.h, kCherryRows) for unfused models
template <bool CR>
void record_plain(HostModel* hm) {
  Recorder<false, CR> rc(hm);
  walk_pass(rc, hm->NV, hm->K);
  for (size_t j = 0; j < rc.loads.size(); ++j) {
    const auto& e = rc.loads[j];
    // prefetchable: its producer store is issued before the previous load (where the prefetch is issued)
    hm->ldsched.push_back(load_word(e.arr, e.slot, j > 0 && e.src >= 0 && e.src < rc.loads[j - 1].t));
  }
  plan_waits(hm, rc.vm_events);
}

// the resolved protein walk with the cherry message table: its stream, counts and wait plan (records and load schedule are
// the plain walk's: verify_walk holds it to them)
void record_cherry_msg(HostModel* hm) {
  Recorder<false, true, true> rc(hm);
  walk_pass(rc, hm->NV, hm->K);
  plan_waits(hm, rc.vm_events, true);
}

// ---- SlotProbe: the workspace transfers of a pass with the record that issues each, in the Recorder's program-order time
struct SlotProbe : RegisterOpsIgnored {
  static constexpr bool kCherryTables = false, kCherryRows = true, kCherryMsg = false, kLdsSlot = false;
  const HostModel* hm;
  long t = 0;
  int cur = -1;
  struct Ev { int arr, slot, v; long t; };
  std::vector<Ev> stores, loads;
  explicit SlotProbe(const HostModel* h) : hm(h) {}
  void rec(int v, int (&r)[16]) { cur = v; copy_record(*hm, v, r); }
  template <int D> void lset(int, int) { ++t; }
  template <int S, int D> void lmul(int, int) { ++t; }
  template <int S> void ldot(int, int, int) { ++t; }
  template <int S, int D, bool TR> void mv(int, int) { ++t; }
  template <int D> void load(int arr, int slot) { loads.push_back({arr, slot, cur, t++}); }
  template <int S> void store(int arr, int slot) { stores.push_back({arr, slot, cur, t++}); }
};
}  // namespace

// Which workspace vectors go through the wave's one LDS slot (cmx_walk.h, kLdsSlot) instead of HBM.  Candidates, at a node
// whose child A is a visited node: (inside) M_a, stored at A's visit and loaded at the node's -- the HBM store stays, the
// outside pass needs it, so the slot saves the load: weight 1; (outside) U_a, stored at the node's visit and loaded at A's --
// neither transfer happens: weight 2.  A candidate occupies the slot from its store to its load in program order; the plan
// is the set of disjoint intervals of largest weight (weighted interval scheduling), written as FLAG_LDS_* bits of the
// records.  Only the 20-state unfused layout has a device backend with a slot; no other model is planned.
void plan_lds_slot(HostModel* hm) {
  for (int v = 0; v < hm->NV; ++v)
    hm->nrec[(size_t)v * 16 + REC_FLAGS] &= ~(FLAG_LDS_M_PUT | FLAG_LDS_M_GET | FLAG_LDS_UA_PUT | FLAG_LDS_U_GET);
  if (!hm->lds_slot || hm->S != 20 || hm->fuse != 1) return;
  SlotProbe pb(hm);
  walk_pass(pb, hm->NV, hm->K);
  std::vector<const SlotProbe::Ev*> st[2];
  st[0].assign(hm->NIW, nullptr);
  st[1].assign(hm->NIW, nullptr);
  for (const auto& e : pb.stores) st[e.arr][e.slot] = &e;   // every vector is written once
  struct Iv { long s, e; int w, put_v, get_v, put_flag, get_flag; };
  std::vector<Iv> iv;
  std::vector<char> m_loaded(hm->NIW, 0);
  auto child_a = [&](int v, int slot) {
    const int* r = &hm->nrec[(size_t)v * 16];
    return r[REC_A + CH_KIND] == KIND_STORED && r[REC_A + CH_SLOT] == slot;
  };
  for (const auto& l : pb.loads) {
    const SlotProbe::Ev* s = st[l.arr][l.slot];
    if (!s || s->t >= l.t) continue;
    if (l.arr == WS_M) {   // the first load of a message is the inside pass's
      if (!m_loaded[l.slot] && child_a(l.v, l.slot)) iv.push_back({s->t, l.t, 1, s->v, l.v, FLAG_LDS_M_PUT, FLAG_LDS_M_GET});
      m_loaded[l.slot] = 1;
    } else if (child_a(s->v, l.slot) && hm->nrec[(size_t)l.v * 16 + REC_SLOT] == l.slot) {
      iv.push_back({s->t, l.t, 2, s->v, l.v, FLAG_LDS_UA_PUT, FLAG_LDS_U_GET});
    }
  }
  std::sort(iv.begin(), iv.end(), [](const Iv& a, const Iv& b) { return a.e < b.e; });
  const size_t n = iv.size();
  std::vector<long> best(n + 1, 0);          // best[i]: largest weight among the first i intervals
  std::vector<size_t> prev(n, 0);            // intervals that end before interval i starts
  for (size_t i = 0; i < n; ++i) {
    prev[i] = (size_t)(std::lower_bound(iv.begin(), iv.begin() + i, iv[i].s, [](const Iv& a, long s) { return a.e < s; }) - iv.begin());
    best[i + 1] = std::max(best[i], best[prev[i]] + iv[i].w);
  }
  for (size_t i = n; i > 0;) {
    if (best[i] == best[i - 1]) { --i; continue; }
    const Iv& x = iv[i - 1];
    hm->nrec[(size_t)x.put_v * 16 + REC_FLAGS] |= x.put_flag;
    hm->nrec[(size_t)x.get_v * 16 + REC_FLAGS] |= x.get_flag;
    i = prev[i - 1];
  }
}

// records -> operator stream + load schedule (with prefetchability) by a dry run of the walk
void record_walk(HostModel* hm) {
  hm->msched.clear();
  hm->msched_r.clear();
  hm->ldsched.clear();
  hm->n_loads = hm->n_stores = hm->n_products = hm->n_leaf_ops = hm->n_products_r = hm->n_leaf_ops_r = 0;
  hm->n_lds_loads = hm->n_lds_stores = hm->n_lds_copies = 0;
  if (hm->cherry_base > 0) {   // the cherry-table walk's own operator stream (same loads and stores)
    Recorder<true, false> rt(hm);
    walk_pass(rt, hm->NV, hm->K);
  }
  if (hm->fuse == 1) record_plain<true>(hm);
  else record_plain<false>(hm);
  hm->msched_m.clear();
  hm->wait_dist_m.clear();
  hm->wait_imm_m.clear();
  hm->msg = HostModel::WalkCounts();
  if (hm->n_cherry_msg > 0) record_cherry_msg(hm);
}

std::vector<PlanEntry> planned_stream(const HostModel& hm, bool resolved) {
  const std::vector<int>& ms = resolved ? hm.msched_m : hm.msched;
  const std::vector<int>& wait_imm = resolved ? hm.wait_imm_m : hm.wait_imm;
  const int n = (int)(ms.size() / 2), C = hm.dC, copies = planned_stream_copies(C);
  const long long unit = (long long)mat_unit(hm.dS) * 8, stride = (long long)hm.MC * unit;   // bytes of an operator, of a class block
  std::vector<PlanEntry> out;
  out.reserve((size_t)copies * (n + 2));
  for (int copy = 0; copy < copies; ++copy) {
    const bool last = copy != 0;            // (planned_stream_copy: copy 0 continues the site block)
    const int step = last ? copy - C : 1;   // classes from this pass's block to the next pass's
    for (int j = 0; j < n + 2; ++j) {
      const int e = j < n ? j : j - n;
      PlanEntry p;
      p.off = ms[2 * (size_t)e] * unit + (j == n ? step * stride : 0);
      p.tx = ms[2 * (size_t)e + 1];
      if (p.tx >= 0 && j == n && last) p.tx = kPlanLeafNoSymbols;
      p.w = wait_imm[(size_t)((e + n - 1) % n)];   // the wait of the op in front: the one that holds this entry when it waits
      out.push_back(p);
    }
  }
  return out;
}

int wait_plan_skew(int entry) { return g_wait_skew.exchange(entry < 0 ? -1 : entry); }

void build_walk_program(HostModel* hm) {
  const int S = hm->S, C = hm->C;
  hm->fuse = (S == 4 && C >= 4) ? (C == 4 ? 4 : 5) : 1;   // (before record_walk: it chooses the cherry visit of the plain stream)
  if (hm->plain) return;
  build_records(hm);
  plan_lds_slot(hm);
  // staged cherry tables only for the class-fused nucleotide layout (16 symbol pairs; 400 for proteins would not fit a stage
  // buffer: their message table is gathered from global memory, below)
  // (a fused model without a single cherry still gets the second stream -- identical to the first: the null's kernel
  // instantiation reads it unconditionally)
  hm->cherry_base = (S == 4 && C >= 4) ? hm->block().cherry_base() : 0;
  // the cherry message table of the 64-site protein walk (cmx_layout.h): every inlined cherry, if the whole table is small enough
  hm->n_cherry_msg = (hm->cherry_msg && cherry_msg_eligible(S, hm->fuse, C, hm->ncherry)) ? hm->ncherry : 0;
  if (hm->cherry_base == 0) hm->ncherry = 0;
  record_walk(hm);
}

}  // namespace cmx
