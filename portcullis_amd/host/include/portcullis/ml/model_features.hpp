// ModelFeatures: the feature side of the filt stage (lib/include/portcullis/ml/model_features.hpp,
// lib/src/model_features.cc:42-235): intron-size threshold, the Markov models trained from junction sets, and the
// feature matrix.  Training counts the windows' k-mers on the device (pjb_markov_train: the tables are bit for bit what the
// models' own train() makes of the same strings); the matrix -- every junction's windows scored against six k-mer and two position
// models -- comes from the device too (pjb_filt_features).  One device context serves a ModelFeatures from its first device call on:
// it holds the genomes of the targets asked for so far, and is opened anew only for junctions on targets it does not hold.
// juncs2FeatureVectors returns a plain row-major matrix whose columns are VAR_NAMES + Junction::JAD_NAMES.  The random-forest
// side: a saved forest (ml/forest.hpp) is walked on the device over the same rows without the matrix leaving it (forestPredict);
// growing a forest from labelled junctions (growForest, pjb_forest_grow) is `train`'s; trainInstance is self-training's: the two sets
// balanced (SMOTE or under-sampling), optionally cleaned (ENN), and grown; the nearest neighbours of both come from pjb_knn.
#pragma once

#include <string>
#include <vector>

#include "../bam/genome_mapper.hpp"
#include "../junction.hpp"
#include "forest.hpp"
#include "markov_model.hpp"
#include "model_bundle.hpp"

struct pjb_ctx;

namespace portcullis {
namespace ml {

extern const std::vector<std::string> VAR_NAMES;  // "Genuine", "rna_usrs", ... "dna_ss" (model_features.hpp:45-60)

class ModelFeatures {
    bam::GenomeMapper* gmap = nullptr;
    std::string genomeFile;
    int device = 0;
    pjb_ctx* ctx = nullptr;               // the device context (deviceContext)
    std::vector<std::string> ctxTargets;  // by target index: the name of the target whose genome the context holds, "" = none

public:
    uint32_t L95 = 0;
    KmerMarkovModel exonModel, intronModel, donorTModel, donorFModel, acceptorTModel, acceptorFModel;
    PosMarkovModel donorPWModel, acceptorPWModel;

    ModelFeatures() {}
    ~ModelFeatures();
    ModelFeatures(const ModelFeatures&) = delete;
    ModelFeatures& operator=(const ModelFeatures&) = delete;

    void setDevice(int d);
    // The context with the genomes of every target a junction of x lies on: the one kept, if it holds them all; else a new one (the old
    // one is destroyed) with the genomes of x's targets.  Self-training calls openDevice(pos + neg) before it trains, so that the
    // genomes are uploaded once for training and for trainInstance.
    pjb_ctx* deviceContext(const JunctionList& x);
    void openDevice(const JunctionList& x) { (void)deviceContext(x); }
    // L95 and the eight models as a file holds them (sizes: the rows trained), and back
    ModelBundle bundle() const;
    void setBundle(const ModelBundle& b);
    bool isCodingPotentialModelEmpty() { return exonModel.size() == 0 || intronModel.size() == 0; }
    bool isPWModelEmpty() { return donorPWModel.size() == 0 || acceptorPWModel.size() == 0; }
    void initGenomeMapper(const std::string& genomeFile);
    uint32_t calcIntronThreshold(const JunctionList& juncs);
    // model_features.cc:77-158 on the device; the models end as their own train() over the same windows would leave them
    void trainCodingPotentialModel(const JunctionList& in);
    void trainSplicingModels(const JunctionList& pass, const JunctionList& fail);
    static std::vector<std::string> featureNames();
    // row-major [x.size()][featureNames().size()] -- ModelFeatures::setRow for every junction of x
    std::vector<double> juncs2FeatureVectors(const JunctionList& x);
    // the columns of that matrix the reference's filter leaves active, in order: the variables of its forests (29, "Genuine" first)
    static const std::vector<int32_t>& activeFeatures();
    // the features table (lib/src/model_features.cc:402-410): a header line, then per junction of x its intron and the active columns of
    // its row of `rows` (full width: [x.size()][featureNames().size()]), default stream formatting
    static void saveFeatures(const std::string& file, const JunctionList& x, const std::vector<double>& rows);
    // ForestProbability::predictInternal over the rows of x: row-major [x.size()][forest.classValues.size()], feature rows and walk on
    // the device in one call (pjb_filt_scores).  featuresOut (optional): the full matrix as juncs2FeatureVectors lays it out, with the
    // device's own columns 0 and 8.  Throws ForestException for a forest that cannot be walked or has other variables.
    // host arithmetic only (pjb_forest_check and the number of variables): throws ForestException for a forest forestPredict would refuse
    static void checkForest(const Forest& forest);
    std::vector<double> forestPredict(const JunctionList& x, const Forest& forest, std::vector<double>* featuresOut = nullptr);
    // ForestProbability grown as trainInstance grows it (lib/src/model_features.cc:422-440) on the rows of x: the feature rows are the
    // device's (pjb_filt_features: what forestPredict walks), column 0 the junctions' isGenuine(), the variables activeFeatures();
    // the forest is grown on the same device (pjb_forest_grow).  featuresOut (optional): the full matrix, as forestPredict returns it.
    // cv (optional): k-fold cross-validation of the same matrix with the same parameters (pjb_forest_cv, one call: the folds' forests
    // grow side by side): fold[i] is the fold that holds x[i] out, pred comes back as [x.size()][2], row i from the forest grown without
    // x[i]'s fold.  The caller has made sure that every fold is held out somewhere and trains on both labels.
    struct CrossValidation {
        int32_t nFolds = 0;
        std::vector<int32_t> fold;
        std::vector<double> pred;
    };
    Forest growForest(const JunctionList& x, int32_t nTrees, uint32_t seed, std::vector<double>* featuresOut = nullptr, CrossValidation* cv = nullptr);
    // ModelFeatures::trainInstance (lib/src/model_features.cc:252-447) for a probability forest.  pos / neg: sorted, genuine flags set.
    // N = |pos| / |neg| - 1.  With smote: N > 0 adds N synthetic rows per negative (Smote, k = 5), N <= 0 erases random negatives until
    // there are no more than positives.  With enn: rows whose 3 nearest neighbours (itself among them) do not all carry their label
    // are dropped; unlike the reference, which sizes the cleaned matrix by the old row count and trains on an uninitialised tail, the
    // matrix then holds the kept rows only.  The matrix -- the label and the 28 active features of sorted(pos + kept negatives), then
    // the synthetic rows with label 0 -- is grown with the reference's seed.  matrixOut (optional): that matrix, row-major, 29 columns.
    // outputPrefix + ".features" is written if saveFeatures (the real rows, before ENN).
    struct TrainOptions {
        int32_t trees = 250;  // DEFAULT_SELFTRAIN_TREES
        bool smote = true, enn = false, saveFeatures = false, verbose = false;
        std::string outputPrefix;
    };
    Forest trainInstance(const JunctionList& pos, const JunctionList& neg, const TrainOptions& o, std::vector<double>* matrixOut = nullptr);
};

}  // namespace ml
}  // namespace portcullis
