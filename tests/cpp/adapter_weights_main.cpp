// Test driver for the per-branch weights of include/comap_mi355x_adapter.hpp and include/comap_mi355x_multigpu.hpp.
//   adapter_weights_main dists <input.bin> <output.bin>
//      getVectors, then with the input's weights: CorrelationStatistic::setWeights + getValuesForAllPairs,
//      CompensationDistance::setWeights + getDistancesForAllPairs, EuclidianDistance::setWeights + getDistancesForAllPairs;
//      a weights vector one entry too long must throw DimensionException for the statistic and for EuclidianDistance;
//      after deleteWeights the statistic is the unweighted one again.
//      output.bin: f64 counts[N*B] (site-major), f64 getWeights()[B], f64 cor[N*N], compDist[N*N], euclid[N*N],
//      f64 corAfterDelete[N*N], int32 dimensionExceptions[2]
//   adapter_weights_main loopback <input.bin> <output.bin> <nranks>
//      LoopbackMultiGpu::computeIntraStats with a weighted CorrelationStatistic and its null; output.bin as
//      tests/cpp/multigpu_main.cpp "loopback": int64 nrows; rows (int64 i, j; f64 stat, prMin, nMin, pValue; int32 rcMin,
//      nSim); int64 nnull; f64 null stat[nnull], nmin[nnull]
// input.bin: tests/cpp/adapter_main.cpp's layout followed by int32 nw; f64 w[nw]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>

#include "comap_mi355x_multigpu.hpp"

template <class T>
static void rd(std::ifstream& f, T* p, size_t n) { f.read(reinterpret_cast<char*>(p), sizeof(T) * n); }
template <class T>
static void wr(std::ofstream& f, const T* p, size_t n) { f.write(reinterpret_cast<const char*>(p), sizeof(T) * n); }

struct Input {
  int32_t h[8];
  uint64_t seed;
  cmx::TreeArrays t;
  cmx::ModelArrays m;
  std::vector<uint8_t> aln;
  cmx::Vdouble w;
};

static Input readInput(const char* path) {
  Input q;
  std::ifstream in(path, std::ios::binary);
  rd(in, q.h, 8);
  rd(in, &q.seed, 1);
  const int nn = q.h[0], T = q.h[1], S = q.h[2], C = q.h[3], N = q.h[4];
  q.t.parent.resize(nn); q.t.branchLengths.resize(nn); q.t.leafOfTaxon.resize(T);
  rd(in, q.t.parent.data(), nn); rd(in, q.t.branchLengths.data(), nn); rd(in, q.t.leafOfTaxon.data(), T);
  q.m.nbStates = S;
  q.m.generator.resize(S * S); q.m.frequencies.resize(S); q.m.rates.resize(C); q.m.rateProbabilities.resize(C);
  rd(in, q.m.generator.data(), S * S); rd(in, q.m.frequencies.data(), S); rd(in, q.m.rates.data(), C);
  rd(in, q.m.rateProbabilities.data(), C);
  q.aln.resize(static_cast<size_t>(T) * N);
  rd(in, q.aln.data(), q.aln.size());
  int32_t nw = 0;
  rd(in, &nw, 1);
  q.w.resize(nw);
  rd(in, q.w.data(), q.w.size());
  if (!in) throw cmx::Exception("input file too short");
  return q;
}

int main(int argc, char** argv) {
  try {
    if (argc == 4 && std::strcmp(argv[1], "dists") == 0) {
      const Input q = readInput(argv[2]);
      const size_t N = q.h[4];
      cmx::Engine eng(q.t, q.m, 0);
      auto mapping = cmx::CoETools::getVectors(eng, q.aln.data(), N);
      cmx::CorrelationStatistic cor;
      cor.setWeights(q.w);
      if (!cor.hasWeights() || cor.getWeights()->size() != q.w.size()) throw cmx::Exception("setWeights did not keep the weights");
      const cmx::Vdouble sc = cor.getValuesForAllPairs(eng, *mapping);
      cmx::CompensationDistance comp;
      comp.setWeights(q.w);
      const cmx::Vdouble dc = comp.getDistancesForAllPairs(eng, *mapping);
      cmx::EuclidianDistance euc;
      euc.setWeights(q.w);
      const cmx::Vdouble de = euc.getDistancesForAllPairs(eng, *mapping);
      int32_t dim[2] = {0, 0};
      cmx::Vdouble bad(q.w);
      bad.push_back(1.);
      cmx::CorrelationStatistic cbad;
      cbad.setWeights(bad);
      try { (void)cbad.getValuesForAllPairs(eng, *mapping); } catch (cmx::DimensionException&) { dim[0] = 1; }
      cmx::EuclidianDistance ebad;
      ebad.setWeights(bad);
      try { (void)ebad.getDistancesForAllPairs(eng, *mapping); } catch (cmx::DimensionException&) { dim[1] = 1; }
      cor.deleteWeights();
      if (cor.hasWeights() || cor.getWeights()) throw cmx::Exception("deleteWeights left weights behind");
      const cmx::Vdouble su = cor.getValuesForAllPairs(eng, *mapping);
      std::ofstream out(argv[3], std::ios::binary);
      wr(out, mapping->data(), N * eng.getNumberOfBranches() * eng.getNumberOfSubstitutionTypes());
      wr(out, comp.getWeights()->data(), comp.getWeights()->size());
      wr(out, sc.data(), sc.size());
      wr(out, dc.data(), dc.size());
      wr(out, de.data(), de.size());
      wr(out, su.data(), su.size());
      wr(out, dim, 2);
      return 0;
    }
    if (argc == 5 && std::strcmp(argv[1], "loopback") == 0) {
      const Input q = readInput(argv[2]);
      const size_t N = q.h[4];
      const int nranks = std::atoi(argv[4]);
      cmx::CorrelationStatistic stat;
      stat.setWeights(q.w);
      cmx::LoopbackMultiGpu mg(q.t, q.m, std::vector<int>(nranks, 0));
      std::vector<cmx::NullDistributionRow> nul;
      const auto rows = mg.computeIntraStats(q.aln.data(), N, nullptr, 0, stat, true, q.seed, q.h[5], q.h[6], q.h[7],
                                             cmx::PairFilters(), &nul);
      std::ofstream out(argv[3], std::ios::binary);
      int64_t nrw = static_cast<int64_t>(rows.size());
      wr(out, &nrw, 1);
      for (const auto& r : rows) {
        int64_t ij[2] = {static_cast<int64_t>(r.i), static_cast<int64_t>(r.j)};
        double v[4] = {r.stat, r.prMin, r.nMin, r.pValue};
        int32_t k[2] = {r.rcMin, r.nSim};
        wr(out, ij, 2); wr(out, v, 4); wr(out, k, 2);
      }
      int64_t nnull = static_cast<int64_t>(nul.size());
      wr(out, &nnull, 1);
      for (const auto& x : nul) wr(out, &x.stat, 1);
      for (const auto& x : nul) wr(out, &x.nMin, 1);
      return 0;
    }
    std::cerr << "usage: adapter_weights_main dists in.bin out.bin | loopback in.bin out.bin nranks\n";
    return 2;
  } catch (cmx::Exception& e) {
    std::cerr << "cmx::Exception: " << e.what() << "\n";
    return 1;
  }
}
