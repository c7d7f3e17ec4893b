// Test driver for cmx::Engine::setLikelihoodScaling / getLikelihoodScaling (include/comap_mi355x_adapter.hpp).
//   adapter_scaling_main <input.bin> <output.bin>
// input.bin: tests/cpp/adapter_main.cpp's layout.  output.bin: int32 before, after (the getter around the setter);
// int32 n_inner; uint8 states[n_inner][N]; f64 probs[n_inner][N][S] of cmx::MarginalAncestralStateReconstruction on the
// scaled engine
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>

#include "comap_mi355x_adapter.hpp"

template <class T>
static void rd(std::ifstream& f, T* p, size_t n) { f.read(reinterpret_cast<char*>(p), sizeof(T) * n); }
template <class T>
static void wr(std::ofstream& f, const T* p, size_t n) { f.write(reinterpret_cast<const char*>(p), sizeof(T) * n); }

int main(int argc, char** argv) {
  if (argc != 3) {
    std::cerr << "usage: adapter_scaling_main <input.bin> <output.bin>\n";
    return 2;
  }
  try {
    std::ifstream in(argv[1], std::ios::binary);
    int32_t h[8];
    uint64_t seed;
    rd(in, h, 8);
    rd(in, &seed, 1);
    const int nn = h[0], T = h[1], S = h[2], C = h[3], N = h[4];
    cmx::TreeArrays t;
    cmx::ModelArrays m;
    t.parent.resize(nn); t.branchLengths.resize(nn); t.leafOfTaxon.resize(T);
    rd(in, t.parent.data(), nn); rd(in, t.branchLengths.data(), nn); rd(in, t.leafOfTaxon.data(), T);
    m.nbStates = S;
    m.generator.resize(S * S); m.frequencies.resize(S); m.rates.resize(C); m.rateProbabilities.resize(C);
    rd(in, m.generator.data(), S * S); rd(in, m.frequencies.data(), S); rd(in, m.rates.data(), C);
    rd(in, m.rateProbabilities.data(), C);
    std::vector<uint8_t> aln(static_cast<size_t>(T) * N);
    rd(in, aln.data(), aln.size());
    if (!in) throw cmx::Exception("input file too short");

    cmx::Engine eng(t, m);
    const int32_t before = eng.getLikelihoodScaling() ? 1 : 0;
    eng.setLikelihoodScaling(true);
    const int32_t after = eng.getLikelihoodScaling() ? 1 : 0;
    cmx::MarginalAncestralStateReconstruction asr(eng, aln, N);
    const std::vector<int>& nodes = asr.getInnerNodes();
    std::ofstream out(argv[2], std::ios::binary);
    const int32_t ni = static_cast<int32_t>(nodes.size());
    wr(out, &before, 1);
    wr(out, &after, 1);
    wr(out, &ni, 1);
    for (const auto& kv : asr.getAncestralSequences())
      for (size_t s : kv.second) { const uint8_t v = static_cast<uint8_t>(s); wr(out, &v, 1); }
    for (int n : nodes) {
      cmx::VVdouble probs;
      asr.getAncestralStatesForNode(n, probs);
      for (const cmx::Vdouble& p : probs) wr(out, p.data(), p.size());
    }
  } catch (const std::exception& e) {
    std::cerr << "error: " << e.what() << "\n";
    return 1;
  }
  return 0;
}
