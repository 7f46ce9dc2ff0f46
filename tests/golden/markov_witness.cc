// Witness for the filt stage's Markov models (own code; make_markov_fixture.py compiles it together with the reference's
// lib/src/markov_model.cc, unchanged).  Reads cases from the file named on the command line and drives the reference's
// KmerMarkovModel / PosMarkovModel through them: the eight models are trained as trainCodingPotentialModel /
// trainSplicingModels train them (model_features.cc:77-159), every row's windows are scored as setRow has them scored
// (calcSplicingScores first, calcCodingPotential only while neither coding model is empty), and every size() and every
// getScore() result is printed, the doubles as their bits.
//
// Input, one item per line (a string may be empty):
//   cases <n>
//   case <name>
//   train <k>        eight blocks in the order exon intron donorT donorF acceptorT acceptorF donorPW acceptorPW,
//   <k strings>      each followed by its strings
//   rows <r>
//   <6 strings>      per row: donor acceptor left_exon left_intron right_intron right_exon
// Output:
//   case <name>
//   trained <8 sizes>
//   row <i> <14 scores>   donorPW acceptorPW donorT donorF acceptorT acceptorF, then exon and intron on left_exon, intron
//                         and exon on left_intron, intron and exon on right_intron, exon and intron on right_exon
//                         ("-" where setRow does not ask)
//   scored <8 sizes>
//
// tests/cpp/markov_witness_check.cc is this program over the project's own header of the same name.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include <portcullis/ml/markov_model.hpp>  // the include path decides whose

using portcullis::ml::KmerMarkovModel;
using portcullis::ml::PosMarkovModel;

static std::string line(std::istream& in) {
    std::string s;
    if (!std::getline(in, s)) {
        std::fprintf(stderr, "markov witness: input ends early\n");
        std::exit(2);
    }
    return s;
}
static size_t count_after(std::istream& in, const char* word) {
    const std::string s = line(in);
    const size_t n = std::strlen(word);
    if (s.compare(0, n, word) != 0 || s.size() < n + 2) {
        std::fprintf(stderr, "markov witness: expected '%s <n>', got '%s'\n", word, s.c_str());
        std::exit(2);
    }
    return (size_t)std::strtoull(s.c_str() + n + 1, nullptr, 10);
}
static void put(double v) {
    uint64_t b;
    std::memcpy(&b, &v, 8);
    std::printf(" %016llx", (unsigned long long)b);
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::ifstream in(argv[1]);
    if (!in) return 2;
    const size_t n_cases = count_after(in, "cases");
    for (size_t c = 0; c < n_cases; c++) {
        const std::string name = line(in).substr(5);
        // constructed first, trained afterwards: the constructors that take the input call a pure virtual function
        KmerMarkovModel exon(5), intron(5), donT(5), donF(5), accT(5), accF(5);
        PosMarkovModel donP(1), accP(1);
        KmerMarkovModel* km[6] = {&exon, &intron, &donT, &donF, &accT, &accF};
        PosMarkovModel* pm[2] = {&donP, &accP};
        for (int m = 0; m < 8; m++) {
            std::vector<std::string> input(count_after(in, "train"));
            for (auto& s : input) s = line(in);
            if (m < 6) km[m]->train(input, 5);
            else pm[m - 6]->train(input, 1);
        }
        std::printf("case %s\ntrained", name.c_str());
        for (int m = 0; m < 6; m++) std::printf(" %zu", km[m]->size());
        std::printf(" %zu %zu\n", donP.size(), accP.size());
        const size_t n_rows = count_after(in, "rows");
        for (size_t r = 0; r < n_rows; r++) {
            std::string w[6];
            for (auto& s : w) s = line(in);
            std::printf("row %zu", r);
            put(donP.getScore(w[0]));
            put(accP.getScore(w[1]));
            put(donT.getScore(w[0]));
            put(donF.getScore(w[0]));
            put(accT.getScore(w[1]));
            put(accF.getScore(w[1]));
            if (exon.size() == 0 || intron.size() == 0) {  // isCodingPotentialModelEmpty, model_features.cc:198
                for (int k = 0; k < 8; k++) std::printf(" -");
            } else {
                put(exon.getScore(w[2]));
                put(intron.getScore(w[2]));
                put(intron.getScore(w[3]));
                put(exon.getScore(w[3]));
                put(intron.getScore(w[4]));
                put(exon.getScore(w[4]));
                put(exon.getScore(w[5]));
                put(intron.getScore(w[5]));
            }
            std::printf("\n");
        }
        std::printf("scored");
        for (int m = 0; m < 6; m++) std::printf(" %zu", km[m]->size());
        std::printf(" %zu %zu\n", donP.size(), accP.size());
    }
    return 0;
}
