// knn_witness.cc -- drives the REFERENCE's own KNN, SMOTE and ENN (lib/src/{knn,smote,enn}.cc of the reference checkout, compiled
// unchanged by make_knn_fixture.py) on matrices read from files, and restates the four lines with which
// ModelFeatures::trainInstance under-samples its negative set.  Build container only; never built by a test or by build().
//
//   knn_witness knn   <matrix.f64> <rows> <cols> <defaultK> <threads> <out.u32>      rows x KNN::getK() indices
//   knn_witness smote <matrix.f64> <rows> <cols> <smoteness> <out.f64>               Smote(5, smoteness, ...): the synthetic rows
//   knn_witness enn   <matrix.f64> <rows> <cols> <labels.u8> <out.u8>                ENN(3, ...), setThreshold(3): the keep mask
//   knn_witness under <size> <keep> <out.u32>                                        the surviving indices; prints the draws that hit `size`
//   knn_witness time  <matrix.f64> <rows> <cols> <defaultK> <threads>                seconds of KNN::execute on stdout
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include <portcullis/ml/enn.hpp>
#include <portcullis/ml/knn.hpp>
#include <portcullis/ml/smote.hpp>

static std::vector<double> read_f64(const char *path, size_t n) {
    std::vector<double> v(n);
    FILE *f = fopen(path, "rb");
    if (!f || fread(v.data(), 8, n, f) != n) {
        fprintf(stderr, "cannot read %zu doubles from %s\n", n, path);
        exit(2);
    }
    fclose(f);
    return v;
}

static void write_all(const char *path, const void *p, size_t bytes) {
    FILE *f = fopen(path, "wb");
    if (!f || fwrite(p, 1, bytes, f) != bytes) {
        fprintf(stderr, "cannot write %s\n", path);
        exit(2);
    }
    fclose(f);
}

int main(int argc, char **argv) {
    const std::string cmd = argc > 1 ? argv[1] : "";
    if ((cmd == "knn" && argc == 8) || (cmd == "time" && argc == 7)) {
        const size_t rows = strtoull(argv[3], 0, 10), cols = strtoull(argv[4], 0, 10);
        std::vector<double> m = read_f64(argv[2], rows * cols);
        portcullis::ml::KNN knn((uint16_t)atoi(argv[5]), (uint16_t)atoi(argv[6]), m.data(), rows, cols);
        const auto t0 = std::chrono::steady_clock::now();
        knn.execute();
        const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (cmd == "time") {
            printf("%.6f\n", sec);
            return 0;
        }
        std::vector<uint32_t> out;
        for (size_t r = 0; r < rows; r++)
            for (uint32_t i : knn.getNNs(r)) out.push_back(i);
        if (out.size() != rows * knn.getK()) return 3;
        write_all(argv[7], out.data(), out.size() * 4);
        printf("%u\n", (unsigned)knn.getK());
        return 0;
    }
    if (cmd == "smote" && argc == 7) {
        const size_t rows = strtoull(argv[3], 0, 10), cols = strtoull(argv[4], 0, 10);
        std::vector<double> m = read_f64(argv[2], rows * cols);
        portcullis::ml::Smote smote(5, (uint16_t)atoi(argv[5]), 1, m.data(), rows, cols); // as trainInstance constructs it
        smote.execute();
        write_all(argv[6], smote.getSynthetic(), smote.getNbSynthRows() * cols * 8);
        printf("%zu\n", smote.getNbSynthRows());
        return 0;
    }
    if (cmd == "enn" && argc == 7) {
        const size_t rows = strtoull(argv[3], 0, 10), cols = strtoull(argv[4], 0, 10);
        std::vector<double> m = read_f64(argv[2], rows * cols);
        std::vector<uint8_t> lab(rows);
        FILE *f = fopen(argv[5], "rb");
        if (!f || fread(lab.data(), 1, rows, f) != rows) return 2;
        fclose(f);
        std::vector<bool> labels(lab.begin(), lab.end()), keep;
        portcullis::ml::ENN enn(3, 1, m.data(), rows, cols, labels); // as trainInstance constructs it
        enn.setThreshold(3);
        const uint32_t discard = enn.execute(keep);
        std::vector<uint8_t> out(keep.begin(), keep.end());
        write_all(argv[6], out.data(), out.size());
        printf("%u\n", discard);
        return 0;
    }
    if (cmd == "under" && argc == 5) {
        const size_t size = strtoull(argv[2], 0, 10), keep = strtoull(argv[3], 0, 10);
        std::vector<std::shared_ptr<uint32_t>> neg2;
        for (size_t i = 0; i < size; i++) neg2.push_back(std::make_shared<uint32_t>((uint32_t)i));
        size_t at_end = 0;
        // model_features.cc:289-294, the positive set's size being `keep`
        std::mt19937 rng(12345);
        while (neg2.size() > keep) {
            std::uniform_int_distribution<int> gen(0, neg2.size()); // uniform, unbiased
            int i = gen(rng);
            at_end += (size_t)i == neg2.size();
            neg2.erase(neg2.begin() + i);
        }
        std::vector<uint32_t> out;
        for (auto &p : neg2) out.push_back(*p);
        write_all(argv[4], out.data(), out.size() * 4);
        printf("%zu\n", at_end);
        return 0;
    }
    fprintf(stderr, "usage: see the head of knn_witness.cc\n");
    return 1;
}
