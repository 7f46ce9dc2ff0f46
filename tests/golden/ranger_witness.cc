// ranger_witness.cc -- the driver behind make_forest_fixture.py: a probability forest grown, saved, loaded back and asked for
// predictions by the reference's own ranger library.  Own code; compiled in a scratch directory against the reference checkout only
// (make_forest_fixture.py does it), never by a test or by build().
//   ranger_witness train <train.f64> <n_rows> <n_trees> <output prefix>      -> <prefix>.forest
//       as ModelFeatures::trainInstance calls Forest::init (lib/src/model_features.cc:422-440), then saveToFile()
//   ranger_witness train <train.f64> <n_rows> <n_trees> <output prefix> <n_cols> <label column> <mtry> <min_node_size> <seed>
//       the same call with the values trainInstance fixes made arguments (mtry and min_node_size 0: ranger's defaults); the name
//       "Genuine" goes to <label column>, the other columns are called x<number>
//   ranger_witness predict <forest file> <test.f64> <n_rows> <pred.f64>      -> n_rows x n_classes predictions
//       as JunctionFilter::forestPredict loads the saved model and runs it (src/junction_filter.cc:660-686)
// The matrices are raw little-endian doubles, row major, one column per name of the header below: "Genuine" and the 28 other
// columns the reference leaves active.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <memory>
#include <string>
#include <vector>

#include <ranger/DataDouble.h>
#include <ranger/ForestProbability.h>

static std::vector<std::string> header() {
    std::vector<std::string> h = {"Genuine", "rna_rel", "rna_rel2raw", "rna_maxmmes", "rna_missmatch", "rna_intron", "dna_minhamm", "dna_pws", "dna_ss"};
    for (int i = 1; i <= 20; i++) {
        char b[16];
        snprintf(b, sizeof b, "JAD%02d", i);
        h.push_back(b);
    }
    return h;
}

static std::vector<std::string> header(size_t cols, size_t label) {
    std::vector<std::string> h;
    for (size_t i = 0; i < cols; i++) h.push_back(i == label ? std::string("Genuine") : "x" + std::to_string(i));
    return h;
}

static Data* loadMatrix(const char* path, size_t rows, const std::vector<std::string>& h = header()) {
    std::vector<double> v(rows * h.size());
    FILE* f = fopen(path, "rb");
    if (!f || fread(v.data(), sizeof(double), v.size(), f) != v.size()) {
        fprintf(stderr, "cannot read %zu x %zu doubles from %s\n", rows, h.size(), path);
        exit(2);
    }
    fclose(f);
    Data* d = new DataDouble(h, rows, h.size());
    bool error = false;
    for (size_t r = 0; r < rows; r++)
        for (size_t c = 0; c < h.size(); c++) d->set(c, r, v[r * h.size() + c], error);
    return d;
}

int main(int argc, char* argv[]) {
    std::vector<std::string> catVars;
    if (argc == 11 && strcmp(argv[1], "train") == 0) {
        const size_t cols = (size_t)atol(argv[6]), label = (size_t)atol(argv[7]);
        if (cols < 2 || label >= cols || strtoul(argv[10], 0, 10) == 0) {
            fprintf(stderr, "train: %zu columns, label column %zu, seed %s (seed 0 makes ranger draw one at random)\n", cols, label, argv[10]);
            return 2;
        }
        Data* d = loadMatrix(argv[2], (size_t)atol(argv[3]), header(cols, label));
        std::shared_ptr<Forest> f = std::make_shared<ForestProbability>();
        f->init("Genuine", MEM_DOUBLE, d, (uint)atoi(argv[8]), argv[5], (uint)atoi(argv[4]), (uint)strtoul(argv[10], 0, 10), 1, IMP_GINI, (uint)atoi(argv[9]), "",
                false, false, catVars, false, AUC, false, 1.0);
        f->setVerboseOut(&std::cerr);
        f->run(false);
        f->saveToFile();
        delete d;
        return 0;
    }
    if (argc == 6 && strcmp(argv[1], "train") == 0) {
        Data* d = loadMatrix(argv[2], (size_t)atol(argv[3]));
        std::shared_ptr<Forest> f = std::make_shared<ForestProbability>();
        f->init("Genuine", MEM_DOUBLE, d, 0, argv[5], (uint)atoi(argv[4]), 1236456789, 1, IMP_GINI, DEFAULT_MIN_NODE_SIZE_PROBABILITY, "", false, false,
                catVars, false, AUC, false, 1.0);
        f->setVerboseOut(&std::cerr);
        f->run(false);
        f->saveToFile();
        delete d;
        return 0;
    }
    if (argc == 6 && strcmp(argv[1], "predict") == 0) {
        const size_t rows = (size_t)atol(argv[4]);
        Data* d = loadMatrix(argv[3], rows);
        std::shared_ptr<Forest> f = std::make_shared<ForestProbability>();
        f->init("Genuine", MEM_DOUBLE, d, 0, "", 250, 1234567890, 1, IMP_GINI, DEFAULT_MIN_NODE_SIZE_PROBABILITY, "", true, true, catVars, false,
                DEFAULT_SPLITRULE, false, 1.0);
        f->setVerboseOut(&std::cerr);
        f->loadFromFile(argv[2]);
        f->run(false);
        FILE* o = fopen(argv[5], "wb");
        for (size_t r = 0; r < rows; r++) fwrite(f->getPredictions()[r].data(), sizeof(double), f->getPredictions()[r].size(), o);
        fclose(o);
        delete d;
        return 0;
    }
    fprintf(stderr, "usage: ranger_witness train <train.f64> <rows> <trees> <prefix> [<cols> <label column> <mtry> <min_node_size> <seed>] | predict <forest> <test.f64> <rows> <pred.f64>\n");
    return 1;
}
