// Host-side model preparation for the engine (internal).  Everything here runs once per context:
// eigen-decomposition of the reversible generator, per (branch, class) transition matrices P = exp(Q r_c t_b),
// joint count matrices P o N^k (SubstitutionCountInterface::getAllNumbersOfSubstitutions, called per branch and
// class inside computeSubstitutionVectors in the reference -- here cached for all replicates), packing into the
// device layouts, and the tree program.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/comap_mi355x.h"
#include "cmx_layout.h"

namespace cmx {

struct HostModel {
  int S = 0, C = 0, K = 0, nn = 0, B = 0, T = 0, NI = 0, root = 0;
  // Device view.  Nucleotide models with >= 4 rate classes are mapped `fuse` classes at a time: the per-class 4-vectors
  // of a site are concatenated into one dS = 4*fuse vector and the per-class operators become the diagonal blocks of
  // one dS x dS operator (class probabilities folded into the count operators), so that one pass of the 20-state
  // machinery does the work of `fuse` class passes.  Otherwise dS = S, dC = C, fuse = 1.
  int dS = 0, dC = 0, fuse = 1;
  // Alphabets other than 4 / 20 states (codon models, CoETools.cpp:95-100): no matrix-core walk is built for them; the
  // plain kernels of cmx_variants.hip map their sites with the states padded to kPlainStates (operators padded with zeros).
  bool plain = false;
  std::vector<int> parent, first_child, next_sib, taxon_of, slot, int_post;
  std::vector<double> blen, pi, rates, probs, cum_pi, cum_probs;
  std::vector<double> P;    // [C][B][S*S] row-major (x -> y)
  std::vector<double> PN;   // [C][B][K][S*S] P o N^k
  std::vector<double> N1;   // [B][K][S*S] N^k at the branch length itself (rate 1): the no-averaging mapping
  std::vector<double> NC;   // [C][B][K][S*S] N^k at r_c t_b (conditional, not P o N): the marginal mapping (nijt.joint = no)
  std::vector<double> MAT;  // [dC][MC][mat_unit(dS)] device matrices: packed P | packed PN | leaf P^T | leaf PN^T | cherry tables (block())
  int MC = 0;               // matrices per (device) class block = block().count(); 0 on the plain path
  std::vector<double> eigV, eigVi, eigLam;   // [NM][S*S], [NM][S*S], [NM][S]: right / left eigenvectors and eigenvalues of the generators
  std::vector<int> model_of;                  // [B] generator of each branch (all 0 for a homogeneous model)
  std::vector<double> CP;   // [C][nn][S][S]    running row sums of P
  std::vector<uint8_t> CPG; // [C][nn][S][32]   guide table of the simulator's inverse-CDF search (cmx_simulate.hip: draw_guided)
  // [nn][sim_node_bytes(S, C)] the same tables as simulate_chain_kernel stages them (cmx_layout.h), thresholds instead of
  // running sums; empty unless sim_has_tables(S, C) (a model without them takes the gather kernel)
  std::vector<uint8_t> simtab;
  std::vector<int> simg;    // [nsimg][16] simulator: groups of four nodes of equal depth (DevModel::simg)
  std::vector<int> simord;  // [nn - 1] the non-root nodes by depth (DevModel::simord)
  int NV = 0;               // visited nodes of the binary device tree (internal, not inlined; pseudo nodes included)
  int NIW = 0;              // workspace slots: NI + pseudo nodes of split multifurcations
  std::vector<int> nrec;    // [NV][16] per-visited-node records (cmx_walk.h)
  std::vector<int> msched;  // operator uses of one class pass in program order: (matrix index, taxon or -1) pairs
  std::vector<int> ldsched; // workspace loads of one class pass: load_word(array, slot, prefetchable)
  // Wait plan (cmx_layout.h; 20-state unfused models, else empty): per op of msched the counted VMEM distance at its wait --
  // the smallest over the op's dynamic instances (a pass inside a site block, a block's first and last pass) -- and the
  // vmcnt immediate taken from it.
  std::vector<int> wait_dist, wait_imm;
  // Cherry tables (cmx_walk.h; class-fused nucleotide models only): an inlined cherry's message and outside visit as rows
  // of 1 + 3 K tables indexed by its two leaves' symbols, for fully resolved alignments (the null's).  The tables follow
  // the leaf operators in a class block (matrix index cherry_base + cherry_of[node] * (1 + 3 K) + table); the walk that
  // uses them has its own operator stream.  ncherry = 0: no tables (proteins, nucleotide models with < 4 classes).
  std::vector<int> cherry_of;   // [nn] cherry index of an inlined cherry node, else -1
  int ncherry = 0, cherry_base = 0;
  std::vector<int> msched_r;    // operator stream of the cherry-table walk; entry (matrix, taxon | cherry_entry(tx1, tx2) | -1)
  ClassBlock block() const { return {NI, K, T, ncherry}; }   // where an operator sits in a class block of MAT
  // per class pass, for traffic / flop accounting (_r: the cherry-table walk)
  size_t n_loads = 0, n_stores = 0, n_products = 0, n_leaf_ops = 0, n_products_r = 0, n_leaf_ops_r = 0;
  // LDS slot of the mapping wave (cmx_walk.h, kLdsSlot).  lds_slot is an input of build_host_model: false = plan nothing.
  // Of n_loads / n_stores, the transfers the slot serves instead of HBM; n_lds_copies: messages written to both.
  bool lds_slot = true;
  size_t n_lds_loads = 0, n_lds_stores = 0, n_lds_copies = 0;
  // Cherry message table (cmx_walk.h, kCherryMsg; cmx_layout.h: cherry_msg_eligible): on fully resolved alignments (the
  // null's) the 64-site protein walk gathers an inlined cherry's message from a device-built table instead of rebuilding it.
  // cherry_msg is an input of build_host_model (false = no table).  n_cherry_msg: cherries with a table, 0 = the resolved walk
  // is the plain one.  msched_m: the resolved walk's operator stream -- the plain one less the cherries' message ops, a
  // gather adds no entry -- with its own wait plan; records, load schedule and LDS-slot plan are shared with the plain walk.
  bool cherry_msg = true;
  int n_cherry_msg = 0;
  std::vector<int> msched_m, wait_dist_m, wait_imm_m;
  struct WalkCounts { size_t loads = 0, stores = 0, products = 0, leaf_ops = 0, lds_loads = 0, lds_stores = 0, lds_copies = 0, gathers = 0; } msg;
  size_t cherry_msg_bytes() const { return cherry_msg_table_bytes(C, n_cherry_msg); }
};

// The walk of a rate-class pass lives in cmx_walk.h.  build_records: the per-node records it reads; record_walk: the
// operator stream and load schedule the device follows (a dry run of the walk) -- both in cmx_host_tree.cpp; verify_walk
// (cmx_host_verify.cpp): the walk run numerically on the host from the device layouts against a direct pruning
// computation (empty string when they agree).
void build_records(HostModel* hm);
void plan_lds_slot(HostModel* hm);   // after build_records, before record_walk: sets the FLAG_LDS_* bits of the records
void record_walk(HostModel* hm);   // ... and the wait plan of the 20-state unfused walk
std::string verify_walk(const HostModel& hm);
// the device stream of a model with a wait plan (cmx_layout.h: PlanEntry), every copy: [planned_stream_copies(dC)][nmv + 2];
// resolved: the stream of the walk with the cherry message table (msched_m), same layout
std::vector<PlanEntry> planned_stream(const HostModel& hm, bool resolved = false);
// test hook (host only, process-wide): the NEXT wait plan built gets the immediate of entry `entry` raised by one -- a wait
// that is too lax, which verify_walk has to refuse before a context exists.  entry < 0 clears; returns the previous value.
// kWaitSkewResolved + k names entry k of the resolved walk's plan (the cherry message table's stream) instead.
constexpr int kWaitSkewResolved = 1 << 20;
int wait_plan_skew(int entry);

// (cmx_host_model.cpp) returns empty string on success, otherwise the error message (status in *code)
std::string build_host_model(const cmx_model* model, const cmx_tree* tree, HostModel* out, int* code);

}  // namespace cmx
