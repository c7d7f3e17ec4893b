// The layouts host and device agree on (internal).  Plain C++17, no HIP: the host model (cmx_host_*.cpp) builds with any
// C++ compiler from this header, the device sources get it through cmx_device.h.
#pragma once

namespace cmx {

// device state count of the plain path (alphabets other than 4 / 20 states, up to 64): the largest alphabet a context takes.
// The plain kernels of cmx_variants.hip run at this many states and simulate_continuous_kernel keeps one row of the
// transition matrix of this length per thread.
constexpr int kPlainStates = 64;

// The tables of the null's LDS simulator (cmx_simulate.hip: simulate_chain_kernel), one block per node: [C][S] rows of
// sim_thr_row(S) 32-bit thresholds of the inverse-CDF search, then the [C][S][32] guide bytes.  A row ends in at least
// kSimThrPad thresholds no draw exceeds, so a search reads kSimThrPad entries at a time without a bounds test.
constexpr int kSimThrPad = 4;
constexpr int sim_thr_row(int S) { return (S + kSimThrPad + 3) & ~3; }
constexpr unsigned long sim_node_bytes(int S, int C) { return (unsigned long)C * S * (sim_thr_row(S) * 4 + 32); }   // a multiple of 16
constexpr unsigned long kSimNodeBytesMax = 3ul * 512 * 16;   // three 16-byte pieces per thread of a 512-thread workgroup
// Which models get these tables (HostModel::simtab), and with them simulate_chain_kernel for the null's large launches;
// every other model is drawn by the gather kernel.  Nucleotides are left out: their rows are 512 bytes per node, which
// sit in L1 / L2 anyway, and a barrier per node over cfg4's 511 nodes costs more than gathering does.
constexpr bool sim_has_tables(int S, int C) { return S > 4 && sim_node_bytes(S, C) <= kSimNodeBytesMax; }

// Ambiguous symbols (alignment codes >= S) are served from extra rows S .. S+A-1 appended to every transposed leaf
// operator: row S+a = sum of the rows of the states compatible with ambiguity id a (filled per call from the caller's
// mask table, default "every state").  A = 12 for nucleotides (IUPAC + gap), 4 for proteins (B, Z, J, X/gap).
constexpr int max_ambig(int S) { return S == 4 ? 12 : 4; }
// A transposed leaf operator is read row by row, the row named by a site's symbol: sixteen sites of a lane group read
// sixteen rows at once.  With rows of S doubles (40 dwords for S = 20, 32 for the class-fused 16) rows 8 (2) apart fall
// on the same LDS banks -- 61 % of the mapping kernel's LDS cycles were bank conflicts.  One double of padding per row
// (42 / 34 dwords) moves the period to 32 rows: no two rows of an operator share a bank.
constexpr int leaf_row_stride(int S) { return S + 1; }             // doubles per row of a transposed leaf operator
constexpr int mat_unit(int S) { return (S + max_ambig(S)) * leaf_row_stride(S); }   // doubles per device matrix
// The column of device state X in a row of a leaf operator or cherry table: state-in-tile major, so that the values one
// lane of the matrix-core layout needs from a row are contiguous.
constexpr int leaf_col(int X, int dS) { return (X % 4) * (dS / 4) + X / 4; }

// A packed SxS product operator is S/4 x S/4 tiles of 4x4 doubles, tile (bi, bj) at position bi * (S/4) + bj, element
// (r, c) of a tile at 4 r + c (cmx_host_model.cpp: pack_blocks).  The two matrix instructions of the mapping walk read it
// one double per lane:
//   v_mfma_f64_4x4x4_4b    A slot of lane l = (row l & 3, column l >> 4) of one tile
//   v_mfma_f64_16x16x4     A slot of lane l = (row l & 15, column l >> 4) of a 16x4 panel = four tiles of one tile column
// The byte offset of lane l's A element for input tile i (columns 4 i .. 4 i + 3 of the operator, or of its transpose
// with tr) of the panel of output rows 0 .. 15: a per-lane base plus a compile-time step.
constexpr int mfma_a_tile_offset(int lane, bool tr) {   // inside a tile, both instructions
  return (tr ? 4 * (lane >> 4) + (lane & 3) : 4 * (lane & 3) + (lane >> 4)) * 8;
}
constexpr int mfma16_a_offset(int lane, int i, bool tr, int S) {
  return ((tr ? i * (S / 4) + ((lane & 15) >> 2) : ((lane & 15) >> 2) * (S / 4) + i) * 16) * 8 + mfma_a_tile_offset(lane, tr);
}

// The operators of the wide mapping (cmx_map_wide.hip: the default mapping of the plain path's alphabets, kPlainStates x
// kPlainStates, on v_mfma_f64_16x16x4).  With column = site and k = row = state, the A operand of output panel p (rows 16 p ..
// 16 p + 15) and k-step i (columns 4 i .. 4 i + 3) is (row 16 p + (l & 15), column 4 i + (l >> 4)) in lane l.  Packed, that is
// double l of the 64 consecutive doubles of (p, i): one coalesced 512-byte read per wave and step.  The host packer
// (cmx_api_map.cpp: pack_wide) and the kernels both place an element with this one function.
// S: the states of the shape, kPlainStates or 20 (below).
constexpr int wide_op_offset(int row, int col, int S = kPlainStates) {
  return ((row >> 4) * (S / 4) + (col >> 2)) * 64 + (col & 3) * 16 + (row & 15);
}
constexpr bool wide_op_offset_is_bijection() {
  bool seen[kPlainStates * kPlainStates] = {};
  for (int r = 0; r < kPlainStates; ++r)
    for (int c = 0; c < kPlainStates; ++c) {
      const int o = wide_op_offset(r, c);
      if (o < 0 || o >= kPlainStates * kPlainStates || seen[o]) return false;
      seen[o] = true;
    }
  return true;
}
// what the kernels rely on: lane l's element of step (p, i) lies at (step's first double) + l
constexpr bool wide_op_offset_is_lane_major() {
  for (int p = 0; p < kPlainStates / 16; ++p)
    for (int i = 0; i < kPlainStates / 4; ++i)
      for (int l = 0; l < 64; ++l)
        if (wide_op_offset(16 * p + (l & 15), 4 * i + (l >> 4)) != wide_op_offset(16 * p, 4 * i) + l) return false;
  return true;
}
static_assert(kPlainStates == 64, "wide_op_offset: four panels of sixteen k-steps");
static_assert(wide_op_offset_is_bijection(), "wide_op_offset must be a bijection onto 64 x 64");
static_assert(wide_op_offset_is_lane_major() && wide_op_offset(0, 0) == 0, "a step's A operand is 64 consecutive doubles, lane-major");
// The same for the 20-state shape of the wide mapping (20-state models under likelihood scaling): two output panels of 16
// rows and five k-steps.  An operator is packed as kWide20Rows x 20 with rows 20 .. 31 zero, so that a panel is a whole
// instruction; 640 doubles instead of 400.
constexpr int kWide20Rows = 32;
constexpr int wide20_op_offset(int row, int col) { return wide_op_offset(row, col, 20); }
constexpr bool wide20_op_offset_is_bijection() {
  bool seen[kWide20Rows * 20] = {};
  for (int r = 0; r < kWide20Rows; ++r)
    for (int c = 0; c < 20; ++c) {
      const int o = wide20_op_offset(r, c);
      if (o < 0 || o >= kWide20Rows * 20 || seen[o]) return false;
      seen[o] = true;
    }
  return true;
}
constexpr bool wide20_op_offset_is_lane_major() {
  for (int p = 0; p < kWide20Rows / 16; ++p)
    for (int i = 0; i < 20 / 4; ++i)
      for (int l = 0; l < 64; ++l)
        if (wide20_op_offset(16 * p + (l & 15), 4 * i + (l >> 4)) != wide20_op_offset(16 * p, 4 * i) + l) return false;
  return true;
}
static_assert(wide20_op_offset_is_bijection(), "wide20_op_offset must be a bijection onto 32 x 20");
static_assert(wide20_op_offset_is_lane_major() && wide20_op_offset(0, 0) == 0, "a step's A operand is 64 consecutive doubles, lane-major");

// A class block of HostModel::MAT / DevModel::MAT: per device class one run of count() matrices of mat_unit doubles.
// `which` names an operator of a branch as in cmx_walk.h: OPER_P (< 0) = transition matrix, k >= 0 = count operator k.
//   [0, NI)                        P of internal edges, 4x4-block packed (matrix-vector products), by operator slot
//   [NI, NI + NI*K)                P o N^k of internal edges, packed, index slot*K + k
//   [first_leaf(), + T)            P of leaf edges transposed, [z][x] = P[x][z] (per-lane row gather by observed symbol)
//   [.., + K*T)                    P o N^k of leaf edges transposed, index k*T + taxon
//   [cherry_base(), + ncherry*(1+3K))  cherry tables of the class-fused nucleotide layout (cmx_walk.h), 16 rows (symbol pair) each
struct ClassBlock {
  int NI, K, T, ncherry;
  constexpr int internal(int slot, int which) const { return which < 0 ? slot : NI + slot * K + which; }
  constexpr int first_leaf() const { return NI + NI * K; }
  constexpr int leaf(int taxon, int which) const { return which < 0 ? first_leaf() + taxon : first_leaf() + T + which * T + taxon; }
  constexpr int cherry_base() const { return first_leaf() + T + K * T; }
  constexpr int cherry(int cherry_index, int table) const { return cherry_base() + cherry_index * (1 + 3 * K) + table; }
  constexpr int count() const { return cherry_base() + ncherry * (1 + 3 * K); }
};

// Operator stream entry of a cherry-table op: the taxa of the cherry's two leaves beside the flag (a leaf op's entry is
// its taxon, a product's -1).  A taxon has 15 bits: a tree has at most 65535 nodes (build_host_model), so a binary tree
// at most 32768 leaves.
constexpr int kCherryFlag = 0x40000000;
constexpr int cherry_entry(int taxon1, int taxon2) { return kCherryFlag | taxon1 | (taxon2 << 15); }
constexpr int cherry_taxon1(int entry) { return entry & 0x7fff; }
constexpr int cherry_taxon2(int entry) { return (entry >> 15) & 0x7fff; }

// ---- Cherry message table of the 64-site protein walk on resolved alignments (cmx_walk.h, kCherryMsg).  Per
// device class and inlined cherry 400 rows, row 20 s1 + s2 = the message M_c = P_c (P_l1[:, s1] o P_l2[:, s2]) of the
// cherry whose leaves show the symbols s1 and s2, written by the walk's own code (cmx_map.hip: cherry_msg_kernel).  A row
// is laid out for the lane that gathers it: quad q = lane >> 4 holds the states 4 sb + q, sb = 0 .. 4, consecutively in a
// 48-byte slot (40 used) -- two 16-byte loads and one 8-byte load per site group, each naturally aligned.
// Tables are ordered [cherry][class]; the device buffer starts with a node index of nn ints -- the cherry index of an inlined
// cherry's node, the alignment row of a leaf, -1 elsewhere -- which the gather reads through the scalar cache (the walk's
// records name tree nodes), padded to cherry_msg_header_bytes.
constexpr int kCherryMsgPairs = 400, kCherryMsgQuadBytes = 48, kCherryMsgRowBytes = 4 * kCherryMsgQuadBytes;
constexpr unsigned long kCherryMsgTableBytes = (unsigned long)kCherryMsgPairs * kCherryMsgRowBytes;   // one cherry, one class
constexpr unsigned long cherry_msg_table_bytes(int C, int cherries) { return (unsigned long)C * cherries * kCherryMsgTableBytes; }
constexpr unsigned long cherry_msg_header_bytes(int nn) { return ((unsigned long)nn * 4 + 255) / 256 * 256; }
// where state x of row `pair` sits in a table, in doubles
constexpr int cherry_msg_offset(int pair, int x) { return (pair * kCherryMsgRowBytes + (x % 4) * kCherryMsgQuadBytes) / 8 + x / 4; }
// The largest table a model gets (C x cherries x 76 800 bytes); a model over it walks the plain stream.  The gathers are
// served from L2 and the Infinity Cache (256 MiB): an eighth of the latter leaves the operators, the workspace traffic and
// the alignments their room.  Only the benchmark's size, 5.5 MB, has been measured.
constexpr unsigned long kCherryMsgMaxBytes = 32ul << 20;
// VMEM instructions of one gather: the two symbols, then per site group two 16-byte loads and one 8-byte load.  None is
// counted in the wait plan (an uncounted instruction behind a request only makes the planned wait stricter).
constexpr int kCherryMsgLoads = 2 + 4 * 3;
constexpr bool cherry_msg_eligible(int S, int fuse, int C, int cherries) {
  return S == 20 && fuse == 1 && cherries > 0 && cherry_msg_table_bytes(C, cherries) <= kCherryMsgMaxBytes;
}

// ---- Wait plan of the 64-site protein walk (20 states, unfused; cmx_host_tree.cpp: plan_waits).  An op waits
// for its operator with s_waitcnt vmcnt(n), n = the counted VMEM instructions the walk issues between the operator's request
// and that wait: kPlanRows DMA rows of the next request (+ 1 with symbols) and kPlanVec per workspace vector moved through HBM
// in between.  That count is a function of the tree, the LDS-slot plan and the place in the stream: the host records it per
// stream entry and the device reads the immediate from the entry.
constexpr int kPlanRows = 4, kPlanVec = 10;
// the immediate for a counted distance: what the run-time count of the other mapping kernels (cmx_map.hip: wait_vm<20, 20>)
// chooses -- every distance up to a request's own instructions is exact, above that the multiples of a vector, and the
// counter's reach ends at three vectors.  A smaller immediate than the distance only waits for more.
constexpr int planned_wait_imm(int distance) {
  const int v = distance % kPlanVec < 7 ? distance % kPlanVec : 6, q = distance / kPlanVec;
  return q <= 2 ? q * kPlanVec + v : 3 * kPlanVec;
}
// The immediates the device can dispatch on: a product waits with nothing newly issued (multiples of a vector), a leaf op
// behind its own request (its rows, + 1 with symbols).  Every distance the walk can produce maps into its op's set; a plan
// with another immediate is refused (verify_walk) and never uploaded.
constexpr bool planned_wait_dispatchable(int imm, bool leaf) {
  if (!leaf) return imm == 0 || imm == 10 || imm == 20 || imm == 30;
  return imm == 4 || imm == 5 || imm == 14 || imm == 15 || imm == 24 || imm == 25 || imm == 30;
}
// Entry of the planned device stream (one 16-byte scalar load per op): entry j describes op j of a class pass and carries
// the wait of the op in front of it, which is the op that holds entry j when it waits.
//   off  byte offset of op j's operator from the base of the pass's class block (one 64-bit scalar add)
//   tx   symbol row of a leaf op, kPlanProduct for a product, kPlanLeafNoSymbols for a leaf op whose symbols are not
//        requested with its operator (op 0 of the next site block: other sites)
//   w    the vmcnt immediate of op j - 1's wait
// A pass reads entries 0 .. nmv + 1: entry nmv is op 0 of the pass that follows (requested by the last op, so its offset
// carries the distance between the two class blocks), entry nmv + 1 is op 1 of that pass, relative to the new base.  The
// stream is stored once per possible successor of a pass (planned_stream_copy): which copy a pass reads is decided at the
// pass boundary, and nothing in the per-op path knows about the wrap.
struct PlanEntry {
  long long off;
  int tx, w;
};
static_assert(sizeof(PlanEntry) == 16, "one s_load_dwordx4 per op");
constexpr int kPlanProduct = -1, kPlanLeafNoSymbols = -2;
// copy 0: the pass that follows is the next class of the same site block (symbols requested); copy 1 + (C - 1) + d: the
// pass is the block's last one and the next block starts d classes further (d = -(C - 1) .. C - 1)
constexpr int planned_stream_copies(int C) { return 2 * C; }
constexpr int planned_stream_copy(int C, bool last_of_block, int class_step) { return last_of_block ? C + class_step : 0; }

// Load-schedule word of a workspace load: bit 31 prefetchable, bit 30 array (WS_M / WS_U), low 24 bits slot
constexpr int load_word(int arr, int slot, bool prefetchable) {
  return (int)((unsigned)slot | (arr ? 0x40000000u : 0u) | (prefetchable ? 0x80000000u : 0u));
}
constexpr int load_word_array(int w) { return (w >> 30) & 1; }
constexpr int load_word_slot(int w) { return w & 0xffffff; }

}  // namespace cmx
