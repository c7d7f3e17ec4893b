// Dumps what build_host_model makes of a list of (tree, model) cases: per case the error message and status code, or a
// length and a 64-bit digest of the bytes of every field of HostModel, one line per field.  Links the host-model sources
// only (cmx_host_*.cpp): no library, no HIP.  scripts/compare_host_model.py builds it against two source directories and
// compares the lines; tests/test_host_model_cpp.py builds it with plain g++ (tests/host_model_cases.py writes the file).
//
//   host_model_dump CASES                 every case of the file
//   host_model_dump --time N CASES NAME   median wall time in ms of N builds of case NAME
//
// Case file: whitespace-separated tokens.
//   tree NAME  { nnodes N | ntaxa T | parent n v.. | blen n v.. | lot n v.. }  end
//   model NAME { nstates S | nclasses C | ntypes K | count_method m | clamp_negative c | nmodels M |
//                Q n v.. | pi | rates | probs | Bk | naive_weights | Qs | pis | Bks | root_freqs n v.. }  end
//   case NAME TREE MODEL lds_slot [mob n v..] ;
// An array that is not named stays NULL.  Doubles are C hex floats.
#include "cmx_host_model.h"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <map>
#include <string>
#include <vector>

namespace {

struct Tree { int nnodes = 0, ntaxa = 0; std::map<std::string, std::vector<int>> iv; std::map<std::string, std::vector<double>> dv; };
struct Model { std::map<std::string, int> s; std::map<std::string, std::vector<double>> dv; };
struct Case { std::string name, tree, model; int lds_slot = 1; bool has_mob = false; std::vector<int> mob; };

std::vector<std::string> g_tok;
size_t g_at = 0;
const std::string& next() {
  if (g_at >= g_tok.size()) { std::fprintf(stderr, "case file ends inside a definition\n"); std::exit(2); }
  return g_tok[g_at++];
}
std::vector<int> ints() { std::vector<int> v((size_t)std::atol(next().c_str())); for (int& x : v) x = std::atoi(next().c_str()); return v; }
std::vector<double> doubles() { std::vector<double> v((size_t)std::atol(next().c_str())); for (double& x : v) x = std::strtod(next().c_str(), nullptr); return v; }

uint64_t digest(const void* p, size_t bytes) {   // FNV-1a
  uint64_t h = 0xcbf29ce484222325ull;
  for (size_t i = 0; i < bytes; ++i) h = (h ^ static_cast<const unsigned char*>(p)[i]) * 0x100000001b3ull;
  return h;
}
template <class T> void array(const char* name, const char* type, const std::vector<T>& v) {
  std::printf("%s %s %zu %016llx\n", name, type, v.size(), (unsigned long long)digest(v.data(), v.size() * sizeof(T)));
}
template <class T> void scalar(const char* name, T v) {
  const long long x = (long long)v;
  std::printf("%s int 1 %016llx %lld\n", name, (unsigned long long)digest(&x, sizeof(x)), x);
}

template <class T> const T* ptr(const std::map<std::string, std::vector<T>>& m, const char* k) {
  auto it = m.find(k);
  return it == m.end() ? nullptr : it->second.data();
}
int num(const std::map<std::string, int>& m, const char* k) { auto it = m.find(k); return it == m.end() ? 0 : it->second; }

std::string build(const Tree& t, const Model& m, const Case& c, cmx::HostModel* hm, int* code) {
  cmx_tree ct{};
  ct.nnodes = t.nnodes; ct.ntaxa = t.ntaxa;
  ct.parent = ptr(t.iv, "parent"); ct.blen = ptr(t.dv, "blen"); ct.leaf_of_taxon = ptr(t.iv, "lot");
  cmx_model cm{};
  cm.nstates = num(m.s, "nstates"); cm.nclasses = num(m.s, "nclasses"); cm.ntypes = num(m.s, "ntypes");
  cm.count_method = num(m.s, "count_method"); cm.clamp_negative = num(m.s, "clamp_negative"); cm.nmodels = num(m.s, "nmodels");
  cm.Q = ptr(m.dv, "Q"); cm.pi = ptr(m.dv, "pi"); cm.rates = ptr(m.dv, "rates"); cm.probs = ptr(m.dv, "probs");
  cm.Bk = ptr(m.dv, "Bk"); cm.naive_weights = ptr(m.dv, "naive_weights");
  cm.Qs = ptr(m.dv, "Qs"); cm.pis = ptr(m.dv, "pis"); cm.Bks = ptr(m.dv, "Bks"); cm.root_freqs = ptr(m.dv, "root_freqs");
  cm.model_of_branch = c.has_mob ? c.mob.data() : nullptr;
  hm->lds_slot = c.lds_slot != 0;
  return cmx::build_host_model(&cm, &ct, hm, code);
}

void dump(const cmx::HostModel& h) {
#define S(f) scalar(#f, h.f)
#define I(f) array(#f, "int", h.f)
#define D(f) array(#f, "f64", h.f)
  S(S); S(C); S(K); S(nn); S(B); S(T); S(NI); S(root); S(dS); S(dC); S(fuse); S(plain);
  I(parent); I(first_child); I(next_sib); I(taxon_of); I(slot); I(int_post);
  D(blen); D(pi); D(rates); D(probs); D(cum_pi); D(cum_probs);
  D(P); D(PN); D(N1); D(NC); D(MAT); S(MC);
  D(eigV); D(eigVi); D(eigLam); I(model_of); D(CP); array("CPG", "u8", h.CPG);
  I(simg); I(simord); S(NV); S(NIW); I(nrec); I(msched); I(ldsched);
  I(cherry_of); S(ncherry); S(cherry_base); I(msched_r);
  S(n_loads); S(n_stores); S(n_products); S(n_leaf_ops); S(n_products_r); S(n_leaf_ops_r);
  S(lds_slot); S(n_lds_loads); S(n_lds_stores); S(n_lds_copies);
#undef S
#undef I
#undef D
}

}  // namespace

int main(int argc, char** argv) {
  int ntime = 0;
  std::string file, only;
  if (argc == 5 && std::string(argv[1]) == "--time") { ntime = std::atoi(argv[2]); file = argv[3]; only = argv[4]; }
  else if (argc == 2) file = argv[1];
  if (file.empty() || (argc == 5 && ntime < 1)) { std::fprintf(stderr, "usage: host_model_dump [--time N] CASES [NAME]\n"); return 2; }
  std::ifstream in(file);
  if (!in) { std::fprintf(stderr, "cannot read %s\n", file.c_str()); return 2; }
  g_tok.assign(std::istream_iterator<std::string>(in), std::istream_iterator<std::string>());
  std::map<std::string, Tree> trees;
  std::map<std::string, Model> models;
  bool timed = false;
  while (g_at < g_tok.size()) {
    const std::string what = next();
    if (what == "tree") {
      Tree& t = trees[next()];
      for (std::string k = next(); k != "end"; k = next()) {
        if (k == "nnodes") t.nnodes = std::atoi(next().c_str());
        else if (k == "ntaxa") t.ntaxa = std::atoi(next().c_str());
        else if (k == "blen") t.dv[k] = doubles();
        else t.iv[k] = ints();
      }
    } else if (what == "model") {
      Model& m = models[next()];
      for (std::string k = next(); k != "end"; k = next()) {
        const bool is_scalar = k == "nstates" || k == "nclasses" || k == "ntypes" || k == "count_method" || k == "clamp_negative" || k == "nmodels";
        if (is_scalar) m.s[k] = std::atoi(next().c_str());
        else m.dv[k] = doubles();
      }
    } else if (what == "case") {
      Case c;
      c.name = next(); c.tree = next(); c.model = next(); c.lds_slot = std::atoi(next().c_str());
      std::string k = next();
      if (k == "mob") { c.has_mob = true; c.mob = ints(); k = next(); }
      if (k != ";" || !trees.count(c.tree) || !models.count(c.model)) { std::fprintf(stderr, "bad case %s\n", c.name.c_str()); return 2; }
      if (ntime && c.name != only) continue;
      const Tree& t = trees[c.tree];
      const Model& m = models[c.model];
      if (ntime) {
        std::vector<double> ms;
        for (int i = 0; i < ntime; ++i) {
          cmx::HostModel hm;
          int code = 0;
          const auto t0 = std::chrono::steady_clock::now();
          const std::string msg = build(t, m, c, &hm, &code);
          ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
          if (!msg.empty()) { std::fprintf(stderr, "%s: %s\n", c.name.c_str(), msg.c_str()); return 1; }
        }
        std::sort(ms.begin(), ms.end());
        std::printf("%s median_ms %.3f min_ms %.3f max_ms %.3f builds %d\n", c.name.c_str(), ms[ms.size() / 2], ms.front(), ms.back(), ntime);
        timed = true;
        continue;
      }
      cmx::HostModel hm;
      int code = 0;
      const std::string msg = build(t, m, c, &hm, &code);
      std::printf("case %s\n", c.name.c_str());
      if (!msg.empty()) std::printf("error %d %s\n", code, msg.c_str());
      else dump(hm);
    } else {
      std::fprintf(stderr, "unexpected token %s\n", what.c_str());
      return 2;
    }
  }
  if (ntime && !timed) { std::fprintf(stderr, "no case named %s\n", only.c_str()); return 2; }
  return 0;
}
