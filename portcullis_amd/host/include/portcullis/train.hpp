// Train: the `train` mode -- a random forest model for `filt --model_file` grown on the device from two junction tables, one of junctions
// known to be genuine and one of junctions known not to be.  It is the last step of the reference's ModelFeatures::trainInstance
// (lib/src/model_features.cc:297-304, 422-440): combine the sets, sort them, make the feature rows, grow a ranger probability forest of
// `trees` trees and save it.  Without --markov the rows are made as `filt --model_file` alone makes them: untrained Markov models, L95 = 0,
// so that model and scoring agree.  With --markov L95 is calcIntronThreshold of the positive set and the Markov models are trained on the
// device from the two sets (coding potential and the true splicing models from the positives, the false ones from the negatives) as
// self-training trains them from its initial sets; the rows carry those columns, and <prefix>.models (ml/model_bundle.hpp) is written
// beside <prefix>.forest for `filt --model_file ... --models_file ...`.  What the reference does before that step and is not built
// (INTEGRATION.md): choosing the sets by layered rules, SMOTE, ENN, the under-sampling, variable importance and the out-of-bag error
// (every row is in bag: there is none to report).
//   --folds k (the reference's own `train` mode, src/train.cc:145-192): k-fold cross-validation of the same rows with the same
// parameters.  Every junction is scored by a forest grown without its fold (pjb_forest_cv: the k forests grow side by side on the
// device), called genuine when its score reaches --threshold, and <prefix>.cv_results holds the folds' confusion matrices and rates
// (ml/performance.hpp) and their means, <prefix>.cv_scores every junction's fold and score.  <prefix>.forest is what it is without
// --folds.  The deviations from the reference (a seeded shuffle, probability forests with a threshold, no NaN, no --markov, no folds
// by default) are in INTEGRATION.md.
#pragma once

#include <string>
#include <vector>

#include "junction_system.hpp"
#include "prepared_files.hpp"

namespace portcullis {

struct TrainException : public PortcullisException {
    explicit TrainException(const std::string& m) : PortcullisException(m) {}
};

const std::string DEFAULT_TRAIN_OUTPUT = "portcullis_train/portcullis";
const int32_t DEFAULT_TRAIN_TREES = 250;
const uint32_t DEFAULT_TRAIN_SEED = 1236456789;  // ModelFeatures::trainInstance
const int32_t DEFAULT_TRAIN_FOLDS = 0;           // no cross-validation (the reference: 5)
const double DEFAULT_TRAIN_THRESHOLD = 0.5;      // JunctionFilter::categorise

class Train {
    PreparedFiles prepData;
    std::string positiveFile, negativeFile, output;
    int32_t trees = DEFAULT_TRAIN_TREES;
    uint32_t seed = DEFAULT_TRAIN_SEED;
    bool saveFeatures = false, verbose = false, markov = false;
    int32_t folds = DEFAULT_TRAIN_FOLDS;
    double threshold = DEFAULT_TRAIN_THRESHOLD;
    int device = 0;

public:
    Train(const std::string& prepDir, const std::string& positiveFile, const std::string& negativeFile, const std::string& output)
        : prepData(prepDir), positiveFile(positiveFile), negativeFile(negativeFile), output(output) {}

    void setTrees(int32_t v) { trees = v; }
    void setSeed(uint32_t v) { seed = v; }
    void setSaveFeatures(bool v) { saveFeatures = v; }
    void setVerbose(bool v) { verbose = v; }
    void setMarkov(bool v) { markov = v; }
    void setDevice(int v) { device = v; }
    void setFolds(int32_t v) { folds = v; }
    void setThreshold(double v) { threshold = v; }

    // The fold that holds out each of n rows: row i starts in fold i % k, then the vector is shuffled by Fisher-Yates from the back
    // (for i = n-1 .. 1: swap v[i] with v[next() % (i + 1)]) with std::mt19937_64 seeded with `seed`.
    static std::vector<int32_t> assignFolds(size_t n, int32_t k, uint32_t seed);

    void train();

    static std::string usage() { return "portcullis_amd train [options] <prep_data_dir> <positive_tab_file> <negative_tab_file>"; }
    static std::string helpMessage();
    static int main(int argc, char* argv[]);
};

}  // namespace portcullis
