// Host model, the self-check (see cmx_host_model.h): the walk of cmx_walk.h run numerically from the device layouts and
// through the recorded streams, against a direct pruning computation on the tree itself.  Plain C++17, no device code.
#include "cmx_host_parts.h"

#include <algorithm>
#include <cmath>

namespace cmx {
namespace {

// ---- Numeric: the pass in plain doubles for one site, operators read from HostModel::MAT in their device layouts
// and selected by the recorded stream exactly as the device selects them; every register starts as NaN.
// CM: the resolved protein walk with the cherry message table -- cset computes what the device's table holds from the host
// matrices, M_c = P_c (P_l1[:, s1] o P_l2[:, s2]), and consumes no stream entry.
template <bool CT, bool CR, bool CM = false>
struct Numeric {
  static constexpr bool kCherryTables = CT, kCherryRows = CR, kCherryMsg = CM;
  static constexpr bool kLdsSlot = !CT;
  std::vector<double> lds;                 // the LDS slot: a fifth vector, NaN until written and again after each read
  int lds_arr = -1, lds_slot = -1;         // its occupant
  const HostModel& hm;
  const ClassBlock mats;
  int dS, NB;
  size_t MU;
  const double* blk;
  std::vector<int> code;                   // symbol per taxon
  std::vector<double> R[4], ws[2], cnt, Lg;
  std::vector<char> counted;
  size_t mi = 0, fi = 0;
  std::string err;
  explicit Numeric(const HostModel& h) : hm(h), mats(h.block()), dS(h.dS), NB(h.dS / 4), MU((size_t)mat_unit(h.dS)), blk(h.MAT.data()) {
    const double nan = std::nan("");
    for (auto& r : R) r.assign(dS, nan);
    lds.assign(dS, nan);
    ws[0].assign((size_t)h.NIW * dS, nan);
    ws[1].assign((size_t)h.NIW * dS, nan);
    cnt.assign((size_t)h.B * h.K, nan);
    counted.assign((size_t)h.B * h.K, 0);
    Lg.assign(h.fuse, nan);
    code.resize(h.T);
    for (int t = 0; t < h.T; ++t) {      // splitmix-style hash of the taxon index: no global RNG state
      uint64_t z = 0x9E3779B97F4A7C15ull * (uint64_t)(t + 1);
      z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; z ^= z >> 31;
      code[t] = (int)(z % (uint64_t)h.S);
    }
  }
  void fail(const std::string& m) { if (err.empty()) err = "tree-walk self-check failed: " + m; }
  void rec(int v, int (&r)[16]) const { copy_record(hm, v, r); }
  // the operator the stream stages for this op; `want` = what the walk asked for
  const std::vector<int>& stream() const { return CM ? hm.msched_m : (CT ? hm.msched_r : hm.msched); }
  int staged(int want_mat, int want_tx) {
    if (2 * mi + 1 >= stream().size()) { fail("more operator uses than the stream holds"); return -1; }
    const int mat = stream()[2 * mi], tx = stream()[2 * mi + 1];
    ++mi;
    if (mat < 0 || mat >= hm.MC) { fail("operator index out of range"); return -1; }
    if (mat != want_mat || tx != want_tx) { fail("op " + std::to_string(mi - 1) + " finds the wrong operator staged"); return -1; }
    return mat;
  }
  int leaf_mat(int leaf, int which) {
    if (leaf < 0 || leaf >= hm.nn || hm.taxon_of[leaf] < 0) { fail("leaf op on a non-leaf"); return -1; }
    const int tx = hm.taxon_of[leaf];
    return staged(mats.leaf(tx, which), tx);
  }
  // cherry tables: row = 4 * symbol(l1) + symbol(l2), columns as in a leaf row
  int cherry_mat(int node, int l1, int l2, int table) {
    if (node < 0 || node >= hm.nn || hm.cherry_of[node] < 0 || table < 0 || table > 3 * hm.K) { fail("cherry op on a node without tables"); return -1; }
    return staged(mats.cherry(hm.cherry_of[node], table), cherry_entry(hm.taxon_of[l1], hm.taxon_of[l2]));
  }
  double cherryrow(int mat, int l1, int l2, int X) const {
    return blk[(size_t)mat * MU + (size_t)(4 * code[hm.taxon_of[l1]] + code[hm.taxon_of[l2]]) * leaf_row_stride(dS) + leaf_col(X, dS)];
  }
  template <int D> void cset(int node, int l1, int l2) {
    if constexpr (CM) {
      if (node < 0 || node >= hm.nn || hm.cherry_of[node] < 0 || hm.slot[node] < 0) return fail("message gather on a node without a table");
      if (l1 < 0 || l1 >= hm.nn || l2 < 0 || l2 >= hm.nn || hm.taxon_of[l1] < 0 || hm.taxon_of[l2] < 0) return fail("message gather on a non-leaf");
      const int ml1 = mats.leaf(hm.taxon_of[l1], OPER_P), ml2 = mats.leaf(hm.taxon_of[l2], OPER_P), mp = mats.internal(hm.slot[node], OPER_P);
      std::vector<double> ab(dS), out(dS, 0.0);
      for (int x = 0; x < dS; ++x) ab[x] = leafrow(ml1, l1, x) * leafrow(ml2, l2, x);
      for (int r = 0; r < dS; ++r)
        for (int c = 0; c < dS; ++c) out[r] += packed(mp, r, c) * ab[c];
      R[D] = out;
      return;
    }
    const int mat = cherry_mat(node, l1, l2, 0);
    if (mat < 0) return;
    for (int x = 0; x < dS; ++x) R[D][x] = cherryrow(mat, l1, l2, x);
  }
  template <int S> void cdot(int node, int l1, int l2, int table, int row) {
    const int mat = cherry_mat(node, l1, l2, table);
    if (mat < 0) return;
    double s = 0;
    for (int x = 0; x < dS; ++x) s += R[S][x] * cherryrow(mat, l1, l2, x);
    count_row(row, s);
  }
  double leafrow(int mat, int leaf, int X) const { return blk[(size_t)mat * MU + (size_t)code[hm.taxon_of[leaf]] * leaf_row_stride(dS) + leaf_col(X, dS)]; }
  double packed(int mat, int r, int c) const {
    if (hm.fuse > 1)   // diagonal tiles only (pack_blocks), the others are exact zeros of the block-diagonal operator
      return r / 4 == c / 4 ? blk[(size_t)mat * MU + (size_t)(r / 4) * 16 + (r % 4) * 4 + c % 4] : 0.0;
    return blk[(size_t)mat * MU + ((size_t)(r / 4) * NB + c / 4) * 16 + (r % 4) * 4 + c % 4];
  }
  void count_row(int row, double v) {
    if (row < 0 || row >= hm.B * hm.K) return fail("count row out of range");
    if (counted[row]) return fail("branch counted twice");
    counted[row] = 1;
    cnt[row] = v;
  }
  template <int D> void lset(int leaf, int which) {
    const int mat = leaf_mat(leaf, which);
    if (mat < 0) return;
    for (int x = 0; x < dS; ++x) R[D][x] = leafrow(mat, leaf, x);
  }
  template <int S, int D> void lmul(int leaf, int which) {
    const int mat = leaf_mat(leaf, which);
    if (mat < 0) return;
    for (int x = 0; x < dS; ++x) R[D][x] = R[S][x] * leafrow(mat, leaf, x);
  }
  template <int S> void ldot(int leaf, int which, int row) {
    const int mat = leaf_mat(leaf, which);
    if (mat < 0) return;
    double s = 0;
    for (int x = 0; x < dS; ++x) s += R[S][x] * leafrow(mat, leaf, x);
    count_row(row, s);
  }
  template <int S, int D, bool TR> void mv(int node, int which) {
    if (node < 0 || node >= hm.nn || hm.slot[node] < 0) return fail("product on a leaf or pseudo branch");
    const int mat = staged(mats.internal(hm.slot[node], which), -1);
    if (mat < 0) return;
    std::vector<double> out(dS, 0.0);
    for (int r = 0; r < dS; ++r)
      for (int c = 0; c < dS; ++c) out[r] += (TR ? packed(mat, c, r) : packed(mat, r, c)) * R[S][c];
    R[D] = out;
  }
  // the next word of the load schedule names this vector
  bool scheduled(int arr, int slot) {
    if (fi >= hm.ldsched.size()) { fail("more workspace loads than scheduled"); return false; }
    const int w = hm.ldsched[fi++];
    if (load_word_array(w) != arr || load_word_slot(w) != slot) { fail("load " + std::to_string(fi - 1) + " names the wrong vector"); return false; }
    return true;
  }
  template <int D> void load(int arr, int slot) {
    if (slot < 0 || slot >= hm.NIW) return fail("workspace slot out of range");
    if (!scheduled(arr, slot)) return;
    R[D].assign(&ws[arr][(size_t)slot * dS], &ws[arr][(size_t)slot * dS] + dS);
  }
  template <int S> void store(int arr, int slot) {
    if (slot < 0 || slot >= hm.NIW) return fail("workspace slot out of range");
    std::copy(R[S].begin(), R[S].end(), &ws[arr][(size_t)slot * dS]);
  }
  template <int D> void lload(int arr, int slot) {
    if (!scheduled(arr, slot)) return;
    if (lds_arr != arr || lds_slot != slot) return fail("load " + std::to_string(fi - 1) + " finds the LDS slot empty or holding another vector");
    R[D] = lds;
    lds.assign(dS, std::nan(""));
    lds_arr = lds_slot = -1;
  }
  template <int S> void lstore(int arr, int slot) {
    if (slot < 0 || slot >= hm.NIW) return fail("workspace slot out of range");
    if (lds_arr >= 0) return fail("the LDS slot is written while it holds a vector nobody has read");
    lds = R[S];
    lds_arr = arr;
    lds_slot = slot;
  }
  template <int S> void lcopy(int arr, int slot) { lstore<S>(arr, slot); }
  template <int D, int S> void mov() { R[D] = R[S]; }
  template <int D, int S> void mul() { for (int x = 0; x < dS; ++x) R[D][x] *= R[S][x]; }
  template <int D, int A, int B> void prod() { for (int x = 0; x < dS; ++x) R[D][x] = R[A][x] * R[B][x]; }
  void mulup() { for (int x = 0; x < dS; ++x) { R[1][x] *= R[3][x]; R[2][x] *= R[3][x]; } }
  template <int D> void setpi() { for (int x = 0; x < dS; ++x) R[D][x] = hm.pi[x % hm.S]; }
  template <int S> void rootl() {
    for (int g = 0; g < hm.fuse; ++g) { double s = 0; for (int x = 0; x < hm.S; ++x) s += hm.pi[x] * R[S][g * hm.S + x]; Lg[g] = s; }
  }
  void dot3(int row) { double s = 0; for (int x = 0; x < dS; ++x) s += R[3][x] * R[1][x] * R[2][x]; count_row(row, s); }
  template <int Rg> void kill() { R[Rg].assign(dS, std::nan("")); }   // a killed register must not be read again
};

// what verify_walk keeps of a numeric pass
struct NumericResult {
  std::string err;
  size_t mi = 0, fi = 0;
  std::vector<int> code;
  std::vector<double> cnt, Lg;
  std::vector<char> counted;
};
template <bool CT, bool CR, bool CM = false>
NumericResult run_numeric(const HostModel& hm) {
  Numeric<CT, CR, CM> nm(hm);
  walk_pass(nm, hm.NV, hm.K);
  return {nm.err, nm.mi, nm.fi, nm.code, nm.cnt, nm.Lg, nm.counted};
}

// ---- WaitModel: the wait plan (cmx_layout.h) against a model of the wave's in-order VMEM queue, the way Numeric models
// the LDS slot's occupant.  The backend follows the walk over consecutive passes as the device's planned walk issues it: a
// leaf op requests the next op's operator (and symbols) and then waits with its planned immediate, a product waits and
// then requests; a workspace vector through HBM is kPlanVec instructions, an LDS-slot transfer none.  A requested stage
// buffer or symbol slot is "not landed" until a wait executes whose immediate is at most the number of counted
// instructions issued behind the request (VMEM completes in order); an op that reads one that has not landed, or one
// requested for another op, and a request into a buffer whose last reader has not run, are refused.  The kernel drains the
// CM: the resolved walk with the cherry message table.  A gather (cset) is kCherryMsgLoads VMEM instructions the plan does
// not count: they enter the queue (`extra`) behind whatever is in flight, so a planned wait executed after them waits for
// at least what it would without them -- positions in the queue are counted + uncounted instructions, immediates and the
// plan's distances are counted ones.  A gather issues no request: the operator of the op behind it was requested by the op
// in front of it and lies in front of the gather's loads.
template <bool CM>
struct WaitModel : RegisterOpsIgnored {
  static constexpr bool kCherryTables = false, kCherryRows = true, kCherryMsg = CM, kLdsSlot = true;
  struct Buf {
    long last = 0, end = 0;   // the request's last instruction (queue position); counted instructions issued when the whole request (symbols too) was out
    long op = -1;             // the dynamic op it was requested for
    bool used = true;         // ... has read it
  };
  const HostModel& hm;
  const std::vector<int>& ms;        // the walk's stream
  const std::vector<int>& wait_imm;  // ... and its plan
  const int n;                // ops of a pass
  long issued = kPlanRows, landed = 0;   // counted instructions so far; queue positions 1 .. landed have completed
  long extra = 0;             // uncounted instructions so far (gathers)
  Buf stage[2], sym[2];
  int par = 0, mi = 0;
  long dyn = 0;               // ops executed so far, over all passes
  bool last_of_block = false;
  std::vector<long> mind;     // smallest modelled distance of each entry
  std::string err;
  explicit WaitModel(const HostModel& h)
      : hm(h), ms(CM ? h.msched_m : h.msched), wait_imm(CM ? h.wait_imm_m : h.wait_imm), n((int)(ms.size() / 2)), mind(n, -1) {
    stage[0] = {kPlanRows, kPlanRows, 0, false};   // the kernel's first request: op 0
  }
  void fail(const std::string& m) { if (err.empty()) err = "wait plan refused: " + m; }
  bool leaf_entry(int i) const { return ms[2 * (size_t)i + 1] >= 0; }
  void rec(int v, int (&r)[16]) const { copy_record(hm, v, r); }
  void begin_block() {
    landed = issued + extra;   // the prologue's drain
    if (leaf_entry(0)) sym[par] = {0, 0, dyn, false};   // ... and its request of op 0's symbols, drained as well
  }
  void begin_pass(bool last) { mi = 0; last_of_block = last; }
  void request_next() {
    const bool more = mi + 1 < n;
    const int next = more ? mi + 1 : 0;
    Buf& b = stage[par ^ 1];
    if (!b.used) return fail("op " + std::to_string(mi) + " requests into a stage buffer whose operator nobody has read");
    issued += kPlanRows;
    b = {issued + extra, issued, dyn + 1, false};
    if (leaf_entry(next) && (more || !last_of_block)) {
      Buf& s = sym[par ^ 1];
      if (!s.used) return fail("op " + std::to_string(mi) + " requests into a symbol slot nobody has read");
      issued += 1;
      s = {issued + extra, issued, dyn + 1, false};
      b.end = issued;
    }
  }
  void wait() {
    if (mi >= n || (size_t)mi >= wait_imm.size()) return fail("more ops than planned waits");
    const int imm = wait_imm[mi];
    if (imm < 0 || imm > 63) return fail("entry " + std::to_string(mi) + ": " + std::to_string(imm) + " is no vmcnt value");
    if (!planned_wait_dispatchable(imm, leaf_entry(mi)))
      return fail("entry " + std::to_string(mi) + ": the device has no wait for vmcnt(" + std::to_string(imm) + ") at this kind of op");
    landed = std::max(landed, issued + extra - imm);
    const long d = issued - stage[par].end;
    if (dyn > 0 && (mind[mi] < 0 || d < mind[mi])) mind[mi] = d;   // (the wave's first op: behind the drain, nothing of a pass in front)
  }
  void use(bool leaf) {
    auto check = [&](Buf& b, const char* what) {
      if (b.op != dyn) return fail("op " + std::to_string(mi) + " finds " + what + " requested for another op");
      if (b.last > landed)
        return fail("op " + std::to_string(mi) + " reads " + what + " that has not landed: vmcnt(" + std::to_string(wait_imm[mi]) + ") with " +
                    std::to_string(issued + extra - b.last) + " instructions issued behind it");
      b.used = true;
    };
    check(stage[par], "a stage buffer");
    if (leaf) check(sym[par], "a symbol slot");
  }
  void end() { par ^= 1; ++mi; ++dyn; }
  void leaf_op() { if (!err.empty()) return; request_next(); wait(); use(true); end(); }
  template <int D> void lset(int, int) { leaf_op(); }
  template <int S, int D> void lmul(int, int) { leaf_op(); }
  template <int S> void ldot(int, int, int) { leaf_op(); }
  template <int S, int D, bool TR> void mv(int, int) { if (!err.empty()) return; wait(); use(false); request_next(); end(); }
  template <int D> void load(int, int) { issued += kPlanVec; }
  template <int S> void store(int, int) { issued += kPlanVec; }
  template <int D> void lload(int, int) {}
  template <int S> void lstore(int, int) {}
  template <int S> void lcopy(int, int) {}
  template <int D> void cset(int, int, int) { extra += kCherryMsgLoads; }
};

// whole: site blocks of all classes, as every launch but the class-split one walks them (the plan's distances are the
// smallest of these instances: checked entry by entry); else one pass per block, the class-split launch
template <bool CM>
std::string check_wait_plan(const HostModel& hm, bool whole) {
  WaitModel<CM> wm(hm);
  const std::vector<int>& wait_dist = CM ? hm.wait_dist_m : hm.wait_dist;
  const std::vector<int>& wait_imm = CM ? hm.wait_imm_m : hm.wait_imm;
  const int C = hm.dC, passes = whole ? C : 1, blocks = whole ? 2 : 2 * std::max(C, 2);
  for (int b = 0; b < blocks; ++b) {
    wm.begin_block();
    for (int c = 0; c < passes; ++c) {
      wm.begin_pass(c + 1 == passes);
      walk_pass(wm, hm.NV, hm.K);
      if (!wm.err.empty()) return wm.err;
      if (wm.mi != wm.n) return "wait plan refused: a pass has " + std::to_string(wm.mi) + " ops, the stream " + std::to_string(wm.n);
    }
  }
  if (!whole) return std::string();
  for (int i = 0; i < wm.n; ++i) {
    if (wait_dist[i] != wm.mind[i])
      return "wait plan refused: entry " + std::to_string(i) + " is planned at distance " + std::to_string(wait_dist[i]) + ", the queue model counts " + std::to_string(wm.mind[i]);
    if (wait_imm[i] != planned_wait_imm((int)wm.mind[i]))
      return "wait plan refused: entry " + std::to_string(i) + " waits with vmcnt(" + std::to_string(wait_imm[i]) + "), distance " + std::to_string(wm.mind[i]) +
             " takes vmcnt(" + std::to_string(planned_wait_imm((int)wm.mind[i])) + ")";
  }
  return std::string();
}

bool close(double a, double b) { return std::fabs(a - b) <= 1e-9 * (std::fabs(a) + std::fabs(b)) + 1e-290; }

// site likelihoods and joint counts of a numeric pass against the direct computation; tables: the cherry-table walk's wording
std::string compare(const NumericResult& nm, const std::vector<double>& Lref, const std::vector<double>& ref, int classes, int K, bool tables) {
  const std::string head = "tree-walk self-check failed: ";
  for (int g = 0; g < classes; ++g)
    if (!close(nm.Lg[g], Lref[g])) return head + (tables ? "site likelihood of the cherry-table walk differs from the direct computation" : "site likelihood differs from the direct computation");
  for (size_t r = 0; r < ref.size(); ++r) {
    if (!nm.counted[r]) return head + (tables ? "the cherry-table walk never counts a branch" : "a branch is never counted");
    if (!close(nm.cnt[r], ref[r])) return head + (tables ? "cherry-table count of branch " : "joint count of branch ") + std::to_string(r / K) + " differs from the direct computation";
  }
  return std::string();
}
}  // namespace

// Runs the walk numerically for one random site of device class 0 and compares site likelihood and all joint counts
// with a direct pruning computation from the row-major hm.P / hm.PN.  Empty string when they agree.
std::string verify_walk(const HostModel& hm) {
  const int S = hm.S, F = hm.fuse, K = hm.K, nn = hm.nn, B = hm.B, root = hm.root;
  const size_t S2 = (size_t)S * S;
  if ((int)hm.nrec.size() != hm.NV * 16) return "tree-walk self-check failed: record table size";
  const NumericResult nm = F == 1 ? run_numeric<false, true>(hm) : run_numeric<false, false>(hm);
  if (!nm.err.empty()) return nm.err;
  if (2 * nm.mi != hm.msched.size()) return "tree-walk self-check failed: unused operators in the stream";
  if (nm.fi != hm.ldsched.size()) return "tree-walk self-check failed: unused workspace loads in the schedule";
  // the wait plan of the 64-site protein walk: a wait that is too lax is a race no test on the device can exclude
  if (S == 20 && F == 1) {
    if (2 * hm.wait_imm.size() != hm.msched.size() || hm.wait_dist.size() != hm.wait_imm.size()) return "wait plan refused: not one wait per operator use";
    for (const bool whole : {true, false}) {
      const std::string bad = check_wait_plan<false>(hm, whole);
      if (!bad.empty()) return bad;
    }
  }
  // the resolved walk with the cherry message table: same site, same reference, the plain walk's loads, stores and LDS slot
  NumericResult nr;
  const bool msg = !hm.msched_m.empty();
  const char* const rtag = " (resolved walk with the cherry message table)";
  if (msg) {
    nr = run_numeric<false, true, true>(hm);
    if (!nr.err.empty()) return nr.err + rtag;
    if (2 * nr.mi != hm.msched_m.size()) return std::string("tree-walk self-check failed: unused operators in the stream") + rtag;
    if (nr.fi != hm.ldsched.size()) return std::string("tree-walk self-check failed: other workspace loads than the plain walk's") + rtag;
    if (hm.msg.loads != hm.n_loads || hm.msg.stores != hm.n_stores || hm.msg.lds_loads != hm.n_lds_loads || hm.msg.lds_stores != hm.n_lds_stores ||
        hm.msg.lds_copies != hm.n_lds_copies)
      return std::string("tree-walk self-check failed: other workspace transfers than the plain walk's") + rtag;
    if (2 * hm.wait_imm_m.size() != hm.msched_m.size() || hm.wait_dist_m.size() != hm.wait_imm_m.size()) return std::string("wait plan refused: not one wait per operator use") + rtag;
    // (whole site blocks only: the class-split launch maps observed alignments, which never take this walk)
    const std::string bad = check_wait_plan<true>(hm, true);
    if (!bad.empty()) return bad + rtag;
  }
  // the cherry-table walk: same site, same reference
  NumericResult nt;
  const bool tables = !hm.msched_r.empty();
  if (tables) {
    nt = run_numeric<true, false>(hm);
    if (!nt.err.empty()) return nt.err + " (cherry-table walk)";
    if (2 * nt.mi != hm.msched_r.size()) return "tree-walk self-check failed: unused operators in the cherry-table stream";
    if (nt.fi != hm.ldsched.size()) return "tree-walk self-check failed: the cherry-table walk loads other workspace vectors";
  }
  const std::vector<int>& code = nm.code;
  std::vector<double> ref((size_t)B * K, 0.0), Lref(F, 0.0);
  for (int g = 0; g < F && g < hm.C; ++g) {   // true classes g of device class 0
    std::vector<double> D((size_t)nn * S), M((size_t)nn * S), U((size_t)nn * S), Up((size_t)nn * S);
    for (int n = 0; n < nn; ++n) {
      double* Dn = &D[(size_t)n * S];
      if (hm.taxon_of[n] >= 0) for (int x = 0; x < S; ++x) Dn[x] = x == code[hm.taxon_of[n]] ? 1.0 : 0.0;
      else { for (int x = 0; x < S; ++x) Dn[x] = 1.0; for (int e : children(hm, n)) for (int x = 0; x < S; ++x) Dn[x] *= M[(size_t)e * S + x]; }
      if (n != root) {
        const double* P = &hm.P[((size_t)g * B + n) * S2];
        for (int x = 0; x < S; ++x) { double s = 0; for (int z = 0; z < S; ++z) s += P[(size_t)x * S + z] * Dn[z]; M[(size_t)n * S + x] = s; }
      }
    }
    for (int x = 0; x < S; ++x) { Lref[g] += hm.pi[x] * D[(size_t)root * S + x]; Up[(size_t)root * S + x] = hm.pi[x]; }
    const double wgt = F > 1 ? hm.probs[g] : 1.0;   // fused: class probabilities are folded into the count operators
    for (int f = nn - 1; f >= 0; --f) {
      if (hm.taxon_of[f] >= 0) continue;
      const std::vector<int> c = children(hm, f);
      for (int n : c) {
        double* Un = &U[(size_t)n * S];
        for (int x = 0; x < S; ++x) Un[x] = Up[(size_t)f * S + x];
        for (int m : c) if (m != n) for (int x = 0; x < S; ++x) Un[x] *= M[(size_t)m * S + x];
        for (int k = 0; k < K; ++k) {
          const double* PN = &hm.PN[(((size_t)g * B + n) * K + k) * S2];
          double tot = 0;
          for (int x = 0; x < S; ++x) { double s = 0; for (int y = 0; y < S; ++y) s += PN[(size_t)x * S + y] * D[(size_t)n * S + y]; tot += Un[x] * s; }
          ref[(size_t)n * K + k] += wgt * tot;
        }
        if (hm.taxon_of[n] < 0) {
          const double* P = &hm.P[((size_t)g * B + n) * S2];
          for (int z = 0; z < S; ++z) { double s = 0; for (int x = 0; x < S; ++x) s += P[(size_t)x * S + z] * Un[x]; Up[(size_t)n * S + z] = s; }
        }
      }
    }
  }
  const int classes = std::min(F, hm.C);
  std::string bad = compare(nm, Lref, ref, classes, K, false);
  if (bad.empty() && tables) bad = compare(nt, Lref, ref, classes, K, true);
  if (bad.empty() && msg) {
    bad = compare(nr, Lref, ref, classes, K, false);
    if (!bad.empty()) bad += rtag;
  }
  return bad;
}

}  // namespace cmx
