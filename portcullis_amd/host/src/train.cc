// Train: see portcullis/train.hpp.
#include <portcullis/train.hpp>

#include <chrono>
#include <cstdio>
#include <fstream>
#include <iomanip>
#include <iostream>
#include <random>
#include <sstream>

#include <portcullis/ml/model_features.hpp>
#include <portcullis/ml/performance.hpp>

#include "../../../include/portcullis_amd.h"
#include "fs_util.hpp"

using std::cout;
using std::endl;
using std::string;

namespace portcullis {

std::vector<int32_t> Train::assignFolds(size_t n, int32_t k, uint32_t seed) {
    std::vector<int32_t> v(n);
    for (size_t i = 0; i < n; i++) v[i] = (int32_t)(i % (size_t)k);
    std::mt19937_64 next(seed);
    for (size_t i = n; i-- > 1;) std::swap(v[i], v[(size_t)(next() % (uint64_t)(i + 1))]);
    return v;
}

// <prefix>.cv_results as the reference lays it out (src/train.cc:153-190): the header, a line per fold (numbered from 1), the ten means
static string cvResults(const JunctionList& x, const std::vector<int32_t>& fold, int32_t folds, const std::vector<double>& score, double threshold) {
    std::vector<uint32_t> tp((size_t)folds, 0), tn(tp), fp(tp), fn(tp);
    for (size_t i = 0; i < x.size(); i++) {
        const bool called = score[i] >= threshold, genuine = x[i]->isGenuine();
        (genuine ? (called ? tp : fn) : (called ? fp : tn))[(size_t)fold[i]]++;
    }
    std::ostringstream out;
    out << "Fold\t" << ml::Performance::longHeader() << "\n";
    ml::PerformanceList perfs;
    for (size_t f = 0; f < (size_t)folds; f++) {
        auto p = std::make_shared<ml::Performance>(tp[f], tn[f], fp[f], fn[f]);
        out << f + 1 << "\t" << p->toLongString() << "\n";
        perfs.add(p);
    }
    perfs.outputMeanPerformance(out);
    return out.str();
}

void Train::train() {
    size_t slash = output.find_last_of('/');
    string outputDir = slash == string::npos ? string(".") : output.substr(0, slash);
    if (outputDir.empty()) outputDir = "/";
    if (trees < 1) throw TrainException("--trees must be at least 1");
    if (folds < 0 || folds == 1) throw TrainException("--folds must be 0 (no cross-validation) or at least 2: " + std::to_string(folds));
    if (!(threshold >= 0.0 && threshold <= 1.0)) throw TrainException("--threshold must lie between 0 and 1");
    if (folds && markov)
        throw TrainException("--folds cannot be combined with --markov: the Markov models would have seen the held-out junctions, and training them fold by fold is not built");
    if (!exists(positiveFile)) throw TrainException("Could not find positive junction file at: " + positiveFile);
    if (!exists(negativeFile)) throw TrainException("Could not find negative junction file at: " + negativeFile);
    if (!exists(prepData.getGenomeFilePath())) throw TrainException("Could not find prepared genome file at: " + prepData.getGenomeFilePath());
    if (!exists(outputDir)) {
        if (!createDirectories(outputDir)) throw TrainException("Could not create output directory at: " + outputDir);
    } else if (!isDirectory(outputDir))
        throw TrainException("File exists with name of suggested output directory: " + outputDir);
    cout << "Loading positive junctions from " << positiveFile << " ...";
    cout.flush();
    JunctionSystem pos(positiveFile);
    cout << " done." << endl << "Found " << pos.getJunctions().size() << " junctions." << endl;
    cout << "Loading negative junctions from " << negativeFile << " ...";
    cout.flush();
    JunctionSystem neg(negativeFile);
    cout << " done." << endl << "Found " << neg.getJunctions().size() << " junctions." << endl << endl;
    if (pos.getJunctions().empty()) throw TrainException("The positive set is empty: " + positiveFile);
    if (neg.getJunctions().empty()) throw TrainException("The negative set is empty: " + negativeFile);
    for (const auto& j : neg.getJunctions())
        if (pos.getJunction(*(j->getIntron())) != nullptr)
            throw TrainException("Junction " + j->getIntron()->toString() + " is in the positive and in the negative set");
    // lib/src/model_features.cc:297-304: positives, then negatives, sorted as one system
    JunctionList training;
    training.reserve(pos.getJunctions().size() + neg.getJunctions().size());
    for (const auto& j : pos.getJunctions()) {
        j->setGenuine(true);
        training.push_back(j);
    }
    for (const auto& j : neg.getJunctions()) {
        j->setGenuine(false);
        training.push_back(j);
    }
    JunctionSystem trainingSystem(training);
    trainingSystem.sort();
    const JunctionList& x = trainingSystem.getJunctions();
    ml::ModelFeatures::CrossValidation cv;
    if (folds) {
        if ((size_t)folds > x.size()) throw TrainException("--folds " + std::to_string(folds) + " is more than the " + std::to_string(x.size()) + " junctions");
        cv.nFolds = folds;
        cv.fold = assignFolds(x.size(), folds, seed);
        std::vector<size_t> held((size_t)folds, 0), heldGenuine((size_t)folds, 0);
        for (size_t i = 0; i < x.size(); i++) {
            held[(size_t)cv.fold[i]]++;
            heldGenuine[(size_t)cv.fold[i]] += x[i]->isGenuine() ? 1 : 0;
        }
        for (size_t f = 0; f < (size_t)folds; f++) {
            const size_t n = x.size() - held[f], genuine = pos.getJunctions().size() - heldGenuine[f];
            if (genuine == 0 || genuine == n)
                throw TrainException("Fold " + std::to_string(f + 1) + " of " + std::to_string(folds) + " would train on " + (genuine ? "positive" : "negative") +
                                     " junctions only (" + std::to_string(n) + " junctions): use fewer folds or another --seed");
        }
    }
    // no device: said before the genome is read, in the words `prep` has for it
    if (pjb_device_count() <= 0)
        throw TrainException("No MI355X (HIP device) is visible: the forest is grown on the GPU and has no CPU fallback.  Run train where the GPU is.");
    cout << "Training a random forest model" << endl << "------------------------------" << endl << endl;
    cout << "Creating feature vector for " << x.size() << " junctions (" << pos.getJunctions().size() << " positive, " << neg.getJunctions().size()
         << " negative)" << endl;
    ml::ModelFeatures mf;  // L95 = 0, untrained Markov models: the rows `filt --model_file` scores ...
    mf.setDevice(device);
    mf.initGenomeMapper(prepData.getGenomeFilePath());
    if (markov) {  // ... or, with --markov, the rows `filt --model_file --models_file` scores: trained as self-training trains on its initial sets
        cout << "Intron length L95 of the positive set: " << mf.calcIntronThreshold(pos.getJunctions()) << endl;
        cout << "Feature learning from training set ...";
        cout.flush();
        mf.openDevice(x);  // (one context for the training and for the forest: every target's genome is uploaded once)
        mf.trainCodingPotentialModel(pos.getJunctions());
        mf.trainSplicingModels(pos.getJunctions(), neg.getJunctions());
        cout << " done." << endl;
    }
    std::vector<double> features;
    cout << "Growing " << trees << " trees" << endl;
    const ml::Forest forest = mf.growForest(x, trees, seed, saveFeatures ? &features : nullptr, folds ? &cv : nullptr);
    ml::ModelFeatures::checkForest(forest);  // (what filt will ask of it)
    if (verbose) cout << "Grown " << forest.treeOff.back() << " nodes in " << forest.nTrees << " trees" << endl;
    if (saveFeatures) {  // lib/src/model_features.cc:402-410: the active columns, default stream formatting
        const string file = output + ".features.training";
        if (verbose) cout << "Saving feature vector to disk: " << file << endl;
        ml::ModelFeatures::saveFeatures(file, x, features);
    }
    forest.save(output + ".forest");
    cout << "Saved forest to file " << output << ".forest" << endl;
    if (markov) {
        mf.bundle().save(output + ".models");
        cout << "Saved L95 and Markov models to file " << output << ".models" << endl;
    }
    if (folds) {
        std::vector<double> score(x.size());
        for (size_t i = 0; i < x.size(); i++) score[i] = 1.0 - cv.pred[i * 2];  // JunctionFilter::categorise
        const string table = cvResults(x, cv.fold, folds, score, threshold);
        cout << endl << "Starting " << folds << "-fold cross validation" << endl << table << "Cross validation completed" << endl << endl;
        std::ofstream resout((output + ".cv_results").c_str());
        resout << table;
        resout.close();
        if (!resout) throw TrainException("Could not write to output file: " + output + ".cv_results");
        cout << "Saved cross validation results to file " << output << ".cv_results" << endl;
        std::ofstream sout((output + ".cv_scores").c_str());
        sout << "refid\tstart\tend\tstrand\tfold\tgenuine\tscore\n";
        for (size_t i = 0; i < x.size(); i++) {
            char num[40];
            snprintf(num, sizeof num, "%.17g", score[i]);
            const Intron& in = *(x[i]->getIntron());
            sout << in.ref.index << "\t" << in.start << "\t" << in.end << "\t" << bam::strandToChar(x[i]->getConsensusStrand()) << "\t" << cv.fold[i] + 1 << "\t"
                 << (x[i]->isGenuine() ? 1 : 0) << "\t" << num << "\n";
        }
        sout.close();
        if (!sout) throw TrainException("Could not write to output file: " + output + ".cv_scores");
        cout << "Saved the held-out scores to file " << output << ".cv_scores" << endl;
    }
}

string Train::helpMessage() {
    return string("Portcullis Train Mode Help\n\n") +
           "Grows the random forest model that `filt --model_file` scores junctions with, on the GPU, from a\n"
           "table of junctions known to be genuine and a table of junctions known not to be.  The model is the\n"
           "file ranger 0.3.8 saves for the same feature rows (byte for byte).\n\n"
           "Usage: " + usage() + "\n\n" +
           "Options:\n"
           "  -o [ --output ] arg (=" + DEFAULT_TRAIN_OUTPUT + ")  Output prefix: <prefix>.forest is written.\n"
           "  --trees arg (=250)                   The number of trees in the forest.\n"
           "  --seed arg (=1236456789)             The forest's seed (the reference's is the default).\n"
           "  --markov                             Train L95 and the Markov models on the two sets first (on the GPU), grow the forest on rows that\n"
           "                                       carry them, and write <prefix>.models for filt --model_file <prefix>.forest --models_file <prefix>.models.\n"
           "  --save_features                      Also write <prefix>.features.training: the feature rows the forest was grown on.\n"
           "  -k [ --folds ] arg (=0)              k-fold cross-validation: every junction is scored by a forest grown without its fold (the k\n"
           "                                       forests grow side by side on the GPU); <prefix>.cv_results gets the folds' TP / TN / FP / FN and\n"
           "                                       rates and their means, <prefix>.cv_scores every junction's fold and score.  0: none; else 2 or more.\n"
           "                                       The folds are dealt round and shuffled with --seed.  Not with --markov.\n"
           "  --threshold arg (=0.5)               With --folds: a held-out junction is called genuine when its score reaches this (0 to 1).\n"
           "  -v [ --verbose ]                     Print extra information\n"
           "  --help                               Produce help message\n\n"
           "Not built: choosing the two sets (the reference's self-training layers), SMOTE, ENN,\n"
           "under-sampling, --genuine (a table of known labels for one junction file: the labels are the two tables\n"
           "here), --fraction, cross-validation with --markov, variable importance and the out-of-bag error (every\n"
           "row is in bag).\n";
}

int Train::main(int argc, char* argv[]) {
    std::vector<string> positional;
    string output = DEFAULT_TRAIN_OUTPUT;
    int32_t trees = DEFAULT_TRAIN_TREES;
    uint32_t seed = DEFAULT_TRAIN_SEED;
    bool saveFeatures = false, verbose = false, help = false, markov = false;
    int32_t folds = DEFAULT_TRAIN_FOLDS;
    double threshold = DEFAULT_TRAIN_THRESHOLD;
    // long options take their value as the next argument or after '='
    for (int i = 1; i < argc; i++) {
        string a = argv[i], inlineValue;
        bool hasInline = false;
        if (a.rfind("--", 0) == 0 && a.find('=') != string::npos) {
            inlineValue = a.substr(a.find('=') + 1);
            a = a.substr(0, a.find('='));
            hasInline = true;
        }
        auto need = [&]() -> string {
            if (hasInline) return inlineValue;
            if (i + 1 >= argc) throw TrainException("Option " + a + " needs a value");
            return argv[++i];
        };
        if (a == "-o" || a == "--output") output = need();
        else if (a == "--trees") trees = (int32_t)std::stol(need());
        else if (a == "--seed") seed = (uint32_t)std::stoul(need());
        else if (a == "--save_features") saveFeatures = true;
        else if (a == "-k" || a == "--folds") folds = (int32_t)std::stol(need());
        else if (a == "--threshold") threshold = std::stod(need());
        else if (a == "--markov") markov = true;
        else if (a == "--devices") (void)need();
        else if (a == "-v" || a == "--verbose") verbose = true;
        else if (a == "--help") help = true;
        else if (!a.empty() && a[0] == '-' && a.size() > 1) throw TrainException("Unknown option: " + a);
        else positional.push_back(a);
    }
    if (help || argc <= 1 || positional.size() < 3) {
        cout << helpMessage() << endl;
        return 1;
    }
    const auto t0 = std::chrono::steady_clock::now();
    cout << "Running portcullis in train mode" << endl << "--------------------------------" << endl << endl;
    Train t(positional[0], positional[1], positional[2], output);
    t.setTrees(trees);
    t.setSeed(seed);
    t.setSaveFeatures(saveFeatures);
    t.setVerbose(verbose);
    t.setMarkov(markov);
    t.setFolds(folds);
    t.setThreshold(threshold);
    t.train();
    const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    std::ios::fmtflags f(cout.flags());
    cout << endl << "Portcullis train completed." << endl << "Total runtime: " << std::fixed << std::setprecision(1) << s << "s" << endl << endl;
    cout.flags(f);
    return 0;
}

}  // namespace portcullis
