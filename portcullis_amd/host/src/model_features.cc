// ModelFeatures: see portcullis/ml/model_features.hpp.  Line numbers refer to lib/src/model_features.cc of the reference.
#include <portcullis/ml/model_features.hpp>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <fstream>
#include <iostream>

#include <portcullis/junction_system.hpp>

#include "../../../include/portcullis_amd.h"
#include "self_train.hpp"

namespace portcullis {
namespace ml {

const std::vector<std::string> VAR_NAMES = {"Genuine",       "rna_usrs",    "rna_dist",      "rna_rel",    "rna_entropy",
                                            "rna_rel2raw",   "rna_maxminanc", "rna_maxmmes", "rna_missmatch", "rna_intron",
                                            "dna_minhamm",   "dna_coding",  "dna_pws",       "dna_ss"};

ModelFeatures::~ModelFeatures() {
    pjb_destroy(ctx);
    delete gmap;
}

void ModelFeatures::setDevice(int d) {
    if (d != device) {  // (a context lives on one device)
        pjb_destroy(ctx);
        ctx = nullptr;
        ctxTargets.clear();
    }
    device = d;
}

void ModelFeatures::initGenomeMapper(const std::string& file) {  // :60-65
    delete gmap;
    genomeFile = file;
    gmap = new bam::GenomeMapper(file);
    gmap->loadFastaIndex();
    pjb_destroy(ctx);  // (the genomes it holds are another file's)
    ctx = nullptr;
    ctxTargets.clear();
}

uint32_t ModelFeatures::calcIntronThreshold(const JunctionList& juncs) {  // :67-75
    std::vector<uint32_t> sizes;
    for (const auto& j : juncs) sizes.push_back(j->getIntronSize());
    std::sort(sizes.begin(), sizes.end());
    L95 = sizes[(size_t)((double)sizes.size() * 0.95)];
    return L95;
}

static void checkRc(pjb_ctx* ctx, int rc, const char* what) {
    if (rc != PJB_OK) throw JunctionException(std::string(what) + ": " + pjb_last_error(ctx));
}

pjb_ctx* ModelFeatures::deviceContext(const JunctionList& x) {
    if (!gmap) throw JunctionException("ModelFeatures: initGenomeMapper was not called");
    int32_t maxRef = 0;
    for (const auto& j : x) maxRef = std::max(maxRef, j->getIntron()->ref.index);
    std::vector<int32_t> lens((size_t)maxRef + 1, 0);
    std::vector<std::string> names((size_t)maxRef + 1);
    for (const auto& j : x) {
        lens[(size_t)j->getIntron()->ref.index] = j->getIntron()->ref.length;
        names[(size_t)j->getIntron()->ref.index] = j->getIntron()->ref.name;
    }
    bool held = ctx != nullptr && names.size() <= ctxTargets.size();
    for (size_t t = 0; held && t < names.size(); t++) held = names[t].empty() || names[t] == ctxTargets[t];
    if (held) return ctx;
    pjb_destroy(ctx);
    ctx = nullptr;
    ctxTargets.clear();
    pjb_config cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.abi_version = PJB_ABI_VERSION;
    cfg.device = device;
    cfg.orientation = PJB_OR_UNKNOWN;
    cfg.strandedness = PJB_SS_UNKNOWN;
    if (pjb_create(&ctx, &cfg) != PJB_OK) throw JunctionException(std::string("pjb_create: ") + pjb_last_error(nullptr));
    checkRc(ctx, pjb_set_refs(ctx, (int32_t)lens.size(), lens.data()), "pjb_set_refs");
    ctxTargets.assign(names.size(), std::string());
    for (size_t t = 0; t < lens.size(); t++) {
        if (names[t].empty()) continue;
        const std::string contig = gmap->fetchContig(names[t]);
        checkRc(ctx, pjb_upload_contig(ctx, (int32_t)t, (const uint8_t*)contig.data(), (int64_t)contig.size()), "pjb_upload_contig");
        ctxTargets[t] = names[t];
    }
    return ctx;
}

// the junctions as device rows
static void fillRows(std::vector<pjb_junction_row>& rows, const JunctionList& x) {
    rows.resize(x.size());
    memset(rows.data(), 0, rows.size() * sizeof(pjb_junction_row));
    for (size_t i = 0; i < x.size(); i++) {
        const Junction& j = *x[i];
        pjb_junction_row& r = rows[i];
        r.refid = j.getIntron()->ref.index;
        r.start = j.getIntron()->start;
        r.end = j.getIntron()->end;
        r.left = j.getLeftAncStart();
        r.right = j.getRightAncEnd();
        r.cons_strand = (uint8_t)j.getConsensusStrand();
        r.nb_raw = j.getNbSplicedAlignments();
        r.nb_dist = j.getNbDistinctAlignments();
        r.nb_ms = j.getNbMultiplySplicedAlignments();
        r.nb_rel = j.getNbReliableAlignments();
        r.entropy = j.getEntropy();
        r.max_min_anc = j.getMaxMinAnchor();
        r.maxmmes = j.getMaxMMES();
        r.hamming5p = j.getHammingDistance5p();
        r.hamming3p = j.getHammingDistance3p();
        // a junction parsed from a .tab has the mean only, at the six digits the writer prints: the integer sum the device divides again
        const double sum = j.getMeanMismatches() * (double)j.getNbSplicedAlignments();
        r.sum_mismatches = sum > 0.0 && sum < 4294967295.0 ? (uint64_t)std::llround(sum) : 0;
        for (int k = 0; k < 20; k++) r.jad[k] = j.getJunctionAnchorDepth((size_t)k);
    }
}

// The windows of the three lists counted on the device (pjb_markov_train: the bases are upper-cased when a genome is uploaded, the
// windows clamped as faidx_fetch_seq clamps them and reverse-complemented on the negative strand).  The tables are the context's until
// its next training.
static pjb_markov_tables trainOnDevice(ModelFeatures& mf, const JunctionList& cp, const JunctionList& pass, const JunctionList& fail) {
    JunctionList x;
    x.reserve(cp.size() + pass.size() + fail.size());
    x.insert(x.end(), cp.begin(), cp.end());
    x.insert(x.end(), pass.begin(), pass.end());
    x.insert(x.end(), fail.begin(), fail.end());
    pjb_ctx* c = mf.deviceContext(x);
    std::vector<pjb_junction_row> rows;
    fillRows(rows, x);
    std::vector<int64_t> idx(x.size());
    for (size_t i = 0; i < idx.size(); i++) idx[i] = (int64_t)i;
    pjb_markov_tables t;
    checkRc(c, pjb_markov_train(c, rows.data(), (int64_t)rows.size(), idx.data(), (int64_t)cp.size(), idx.data() + cp.size(), (int64_t)pass.size(),
                               idx.data() + cp.size() + pass.size(), (int64_t)fail.size(), &t),
            "pjb_markov_train");
    return t;
}

void ModelFeatures::trainCodingPotentialModel(const JunctionList& in) {  // :77-112
    const pjb_markov_tables t = trainOnDevice(*this, in, JunctionList(), JunctionList());
    exonModel.fill(t.models.exon, PJB_KMER_ORDER);
    intronModel.fill(t.models.intron, PJB_KMER_ORDER);
}

void ModelFeatures::trainSplicingModels(const JunctionList& pass, const JunctionList& fail) {  // :114-158
    const pjb_markov_tables t = trainOnDevice(*this, JunctionList(), pass, fail);
    donorPWModel.fill(t.models.donor_pw, 1);
    acceptorPWModel.fill(t.models.acceptor_pw, 1);
    donorTModel.fill(t.models.donor_t, PJB_KMER_ORDER);
    acceptorTModel.fill(t.models.acceptor_t, PJB_KMER_ORDER);
    donorFModel.fill(t.models.donor_f, PJB_KMER_ORDER);
    acceptorFModel.fill(t.models.acceptor_f, PJB_KMER_ORDER);
}

ModelBundle ModelFeatures::bundle() const {
    ModelBundle b;
    b.L95 = L95;
    const double* src[8] = {exonModel.table(),      intronModel.table(),    donorTModel.table(),  donorFModel.table(),
                            acceptorTModel.table(), acceptorFModel.table(), donorPWModel.table(), acceptorPWModel.table()};
    for (size_t m = 0; m < 8; m++)
        if (src[m]) std::copy(src[m], src[m] + (m < ModelBundle::KMER_MODELS ? ModelBundle::KMER_TABLE : ModelBundle::POS_TABLE), b.table(m));
    b.countSizes();
    return b;
}

void ModelFeatures::setBundle(const ModelBundle& b) {
    L95 = b.L95;
    exonModel.fill(b.table(0), PJB_KMER_ORDER);
    intronModel.fill(b.table(1), PJB_KMER_ORDER);
    donorTModel.fill(b.table(2), PJB_KMER_ORDER);
    donorFModel.fill(b.table(3), PJB_KMER_ORDER);
    acceptorTModel.fill(b.table(4), PJB_KMER_ORDER);
    acceptorFModel.fill(b.table(5), PJB_KMER_ORDER);
    donorPWModel.fill(b.table(6), 1);
    acceptorPWModel.fill(b.table(7), 1);
}

std::vector<std::string> ModelFeatures::featureNames() {
    std::vector<std::string> n = VAR_NAMES;
    n.insert(n.end(), Junction::JAD_NAMES.begin(), Junction::JAD_NAMES.end());
    return n;
}

// The context with the genomes of the targets the junctions lie on (the ModelFeatures' own: deviceContext), the junctions as device rows
// and the models as the C ABI takes them: what the feature matrix and the fused forest walk both start from.
namespace {
struct DeviceRun {
    pjb_ctx* ctx = nullptr;
    std::vector<pjb_junction_row> rows;
    pjb_markov_models m;
    void check(int rc, const char* what) const { checkRc(ctx, rc, what); }
};
}  // namespace

static void openRun(DeviceRun& run, ModelFeatures& mf, const JunctionList& x) {
    run.ctx = mf.deviceContext(x);
    fillRows(run.rows, x);
    pjb_markov_models& m = run.m;
    memset(&m, 0, sizeof m);
    m.exon = mf.exonModel.table();
    m.intron = mf.intronModel.table();
    m.donor_t = mf.donorTModel.table();
    m.donor_f = mf.donorFModel.table();
    m.acceptor_t = mf.acceptorTModel.table();
    m.acceptor_f = mf.acceptorFModel.table();
    m.donor_pw = mf.donorPWModel.table();
    m.acceptor_pw = mf.acceptorPWModel.table();
    m.exon_size = (int32_t)mf.exonModel.size();
    m.intron_size = (int32_t)mf.intronModel.size();
    m.donor_pw_size = (int32_t)mf.donorPWModel.size();
    m.acceptor_pw_size = (int32_t)mf.acceptorPWModel.size();
}

// The feature rows of x (not empty), full width: the device's (pjb_filt_features: what forestPredict walks), column 0 the junctions'
// isGenuine().  `run` is opened here and stays the caller's: trainInstance goes on with its context.
static std::vector<double> featureRows(DeviceRun& run, ModelFeatures& mf, const JunctionList& x) {
    const size_t F = PJB_N_FEATURES;
    std::vector<double> rows(x.size() * F, 0.0);
    openRun(run, mf, x);
    run.check(pjb_filt_features(run.ctx, run.rows.data(), (int64_t)run.rows.size(), x[0]->getMeanReadLength(), mf.L95, &run.m, rows.data()), "pjb_filt_features");
    for (size_t i = 0; i < x.size(); i++) rows[i * F] = x[i]->isGenuine() ? 1.0 : 0.0;
    return rows;
}

// full-width rows -> the columns of activeFeatures(), in their order
static std::vector<double> projectActive(const std::vector<double>& rows) {
    const size_t F = PJB_N_FEATURES, n = rows.size() / F;
    const std::vector<int32_t>& active = ModelFeatures::activeFeatures();
    std::vector<double> matrix(n * active.size());
    for (size_t i = 0; i < n; i++)
        for (size_t k = 0; k < active.size(); k++) matrix[i * active.size() + k] = rows[i * F + (size_t)active[k]];
    return matrix;
}

std::vector<double> ModelFeatures::juncs2FeatureVectors(const JunctionList& x) {  // :214-230 with setRow :161-212
    if (!gmap) throw JunctionException("ModelFeatures: initGenomeMapper was not called");
    if (x.empty()) return std::vector<double>();
    DeviceRun run;
    std::vector<double> out = featureRows(run, *this, x);
    for (size_t i = 0; i < x.size(); i++)
        out[i * PJB_N_FEATURES + 8] = x[i]->getMeanMismatches();  // the junction's own value (a row parsed from a .tab has no integer sum)
    return out;
}

void ModelFeatures::saveFeatures(const std::string& file, const JunctionList& x, const std::vector<double>& rows) {
    std::ofstream fout(file.c_str());
    const std::vector<std::string> names = featureNames();
    const std::vector<int32_t>& active = activeFeatures();
    fout << Intron::locationOutputHeader();
    for (const int32_t k : active) fout << "\t" << names[(size_t)k];
    fout << std::endl;
    for (size_t i = 0; i < x.size(); i++) {
        fout << *(x[i]->getIntron());
        for (const int32_t k : active) fout << "\t" << rows[i * names.size() + (size_t)k];
        fout << std::endl;
    }
}

const std::vector<int32_t>& ModelFeatures::activeFeatures() {  // src/junction_filter.cc:246-258 of the reference
    static const std::vector<int32_t> a = [] {
        std::vector<int32_t> v = {0, 3, 5, 7, 8, 9, 10, 12, 13};
        for (int32_t k = 14; k < PJB_N_FEATURES; k++) v.push_back(k);
        return v;
    }();
    return a;
}

void ModelFeatures::checkForest(const Forest& forest) {
    pjb_forest view;
    forest.view(view);
    char msg[200] = "";
    if (pjb_forest_check(&view, msg, (int)sizeof msg) != PJB_OK) throw ForestException(std::string("The forest model cannot be used: ") + msg);
    if ((size_t)forest.nVars != activeFeatures().size())
        throw ForestException("The forest model was trained on " + std::to_string(forest.nVars) + " variables; this filter makes the " +
                              std::to_string(activeFeatures().size()) + " columns the reference leaves active (Genuine and 28 features)");
}

std::vector<double> ModelFeatures::forestPredict(const JunctionList& x, const Forest& forest, std::vector<double>* featuresOut) {
    const size_t nClasses = forest.classValues.size();
    std::vector<double> pred(x.size() * nClasses, 0.0);
    if (featuresOut) featuresOut->assign(x.size() * PJB_N_FEATURES, 0.0);
    if (x.empty()) return pred;
    checkForest(forest);  // (before a device is opened)
    pjb_forest view;
    forest.view(view);
    DeviceRun run;
    openRun(run, *this, x);
    run.check(pjb_forest_load(run.ctx, &view), "pjb_forest_load");
    run.check(pjb_filt_scores(run.ctx, run.rows.data(), (int64_t)run.rows.size(), x[0]->getMeanReadLength(), L95, &run.m, activeFeatures().data(), pred.data(),
                              featuresOut ? featuresOut->data() : nullptr),
              "pjb_filt_scores");
    return pred;
}

Forest ModelFeatures::growForest(const JunctionList& x, int32_t nTrees, uint32_t seed, std::vector<double>* featuresOut, CrossValidation* cv) {
    if (x.empty()) throw ForestException("No junctions to grow a forest on");
    DeviceRun run;
    std::vector<double> rows = featureRows(run, *this, x);
    const std::vector<double> matrix = projectActive(rows);
    pjb_grow_params p;
    memset(&p, 0, sizeof p);
    p.n_trees = nTrees;
    p.seed = seed;
    pjb_grow_result r;
    run.check(pjb_forest_grow(run.ctx, matrix.data(), (int64_t)x.size(), (int32_t)activeFeatures().size(), &p, &r), "pjb_forest_grow");
    if (featuresOut) featuresOut->swap(rows);
    const Forest forest = Forest::fromView(r.forest, r.class_values);  // (a copy: pjb_forest_cv may take the result away)
    if (cv) {
        if (cv->fold.size() != x.size()) throw ForestException("growForest: " + std::to_string(cv->fold.size()) + " fold ids for " + std::to_string(x.size()) + " junctions");
        cv->pred.assign(x.size() * 2, 0.0);
        run.check(pjb_forest_cv(run.ctx, matrix.data(), (int64_t)x.size(), (int32_t)activeFeatures().size(), &p, cv->fold.data(), cv->nFolds, cv->pred.data(), nullptr),
                  "pjb_forest_cv");
    }
    return forest;
}

Forest ModelFeatures::trainInstance(const JunctionList& pos, const JunctionList& neg, const TrainOptions& o, std::vector<double>* matrixOut) {
    using std::cout;
    using std::endl;
    if (pos.empty() || neg.empty()) throw ForestException("trainInstance needs a positive and a negative junction at least");
    const int N = (int)(pos.size() / neg.size()) - 1;  // the number of times to duplicate the negative set
    JunctionList neg2 = neg;
    if (N <= 0 && o.smote) {
        cout << "Undersampling negative set to balance with positive set" << endl;
        neg2.clear();
        for (const size_t i : selftrain::undersample(neg.size(), pos.size())) neg2.push_back(neg[i]);
    }
    if (o.verbose) cout << endl << "Combining positive, negative " << (N > 0 ? "and synthetic negative " : "") << "datasets." << endl;
    JunctionList training;
    training.reserve(pos.size() + neg2.size());
    training.insert(training.end(), pos.begin(), pos.end());
    training.insert(training.end(), neg2.begin(), neg2.end());
    JunctionSystem trainingSystem(training);
    trainingSystem.sort();
    const JunctionList& x = trainingSystem.getJunctions();
    // the feature rows of the real junctions: the device's (what forestPredict walks), column 0 the genuine flag
    const size_t C = activeFeatures().size(), SC = C - 1;
    DeviceRun run;  // (lives on: pjb_knn and pjb_forest_grow below run on its context)
    const std::vector<double> rows = featureRows(run, *this, x);
    std::vector<double> matrix = projectActive(rows);
    auto nearest = [&](const std::vector<double>& m, size_t n, int32_t defaultK, std::vector<uint32_t>& nn) {
        const int32_t k = selftrain::effectiveK(n, defaultK);
        nn.assign(n * (size_t)k, 0);
        run.check(pjb_knn(run.ctx, m.data(), (int64_t)n, (int32_t)SC, k, nn.data()), "pjb_knn");
        return (size_t)k;
    };
    if (N > 0 && o.smote) {
        cout << "Oversampling negative set to balance with positive set using SMOTE" << endl;
        // the negatives' features in the sorted negative set's order: the negatives of x, which the same comparator sorted
        std::vector<double> nm;
        size_t at = 0;
        for (size_t i = 0; i < x.size(); i++) {
            if (x[i]->isGenuine()) continue;
            if (at >= neg.size() || x[i] != neg[at++]) throw ForestException("trainInstance: the negative set is not sorted");
            nm.insert(nm.end(), matrix.begin() + (std::ptrdiff_t)(i * C + 1), matrix.begin() + (std::ptrdiff_t)((i + 1) * C));
        }
        if (at != neg.size()) throw ForestException("trainInstance: a junction is in the positive and in the negative set");
        std::vector<uint32_t> nn;
        const size_t k = nearest(nm, neg.size(), 5, nn);
        const std::vector<double> synthetic = selftrain::smoteSynthesize(nm.data(), neg.size(), SC, nn.data(), k, (uint32_t)N);
        const size_t nSynth = synthetic.size() / SC;
        for (size_t i = 0; i < nSynth; i++) {
            matrix.push_back(0.0);  // not genuine
            matrix.insert(matrix.end(), synthetic.begin() + (std::ptrdiff_t)(i * SC), synthetic.begin() + (std::ptrdiff_t)((i + 1) * SC));
        }
        cout << "Number of synthesized entries: " << nSynth << endl;
    }
    if (o.saveFeatures) {  // :402-410: the real rows (the synthetic ones have no junction)
        const std::string file = o.outputPrefix + ".features";
        if (o.verbose) cout << "Saving feature vector to disk: " << file << endl;
        saveFeatures(file, x, rows);
    }
    if (o.enn) {
        const size_t n = matrix.size() / C;
        std::vector<double> m(n * SC);
        std::vector<char> labels(n);
        size_t p = 0;
        for (size_t i = 0; i < n; i++) {
            labels[i] = matrix[i * C] == 1.0;
            p += labels[i] != 0;
            std::copy(matrix.begin() + (std::ptrdiff_t)(i * C + 1), matrix.begin() + (std::ptrdiff_t)((i + 1) * C), m.begin() + (std::ptrdiff_t)(i * SC));
        }
        cout << "P: " << p << "; N: " << n - p << "; O: 0" << endl;
        cout << endl << "Starting Wilson's Edited Nearest Neighbour (ENN) to clean decision region" << endl;
        std::vector<uint32_t> nn;
        const size_t k = nearest(m, n, 3, nn);
        const std::vector<char> keep = selftrain::ennKeep(nn.data(), n, k, labels, 3);
        std::vector<double> kept;
        size_t pcount = 0, ncount = 0;
        for (size_t i = 0; i < n; i++) {
            if (!keep[i]) continue;
            kept.insert(kept.end(), matrix.begin() + (std::ptrdiff_t)(i * C), matrix.begin() + (std::ptrdiff_t)((i + 1) * C));
            (labels[i] ? pcount : ncount)++;
        }
        cout << "Marked " << pcount + ncount << " to be kept and " << n - pcount - ncount << " to be discarded." << endl;
        cout << "Final training set contains " << pcount << " positive entries and " << ncount << " negative entries" << endl;
        matrix.swap(kept);
    }
    if (matrix.empty()) throw ForestException("trainInstance: ENN left no row to train on");
    if (o.verbose) cout << "Initialising random forest" << endl << "Training" << endl;
    pjb_grow_params gp;
    memset(&gp, 0, sizeof gp);
    gp.n_trees = o.trees;
    gp.seed = 1236456789u;  // the reference's fixed seed
    pjb_grow_result r;
    run.check(pjb_forest_grow(run.ctx, matrix.data(), (int64_t)(matrix.size() / C), (int32_t)C, &gp, &r), "pjb_forest_grow");
    Forest forest = Forest::fromView(r.forest, r.class_values);
    if (matrixOut) matrixOut->swap(matrix);
    return forest;
}

}  // namespace ml
}  // namespace portcullis
