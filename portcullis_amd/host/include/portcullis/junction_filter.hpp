// JunctionFilter: the `filt` stage (src/junction_filter.hpp / .cc:153-596, 753-896 of the reference) for every mode that does not TRAIN
// a model: a saved random-forest model (walked on the device, fused with the feature rows: ModelFeatures::forestPredict), rule files
// (rule_filter.hpp: no Python), the length / canonical / coverage filters, the rescue of junctions found in a reference BED, and the
// .pass / .fail / .ref outputs.  Same setters, same messages, same order of stages.  Self-training -- the reference's default when
// neither a model nor --no_ml is given -- is built behind --self_train <data_dir> (selfTrain(): the layered rule sets choose the
// initial sets, ModelFeatures::trainInstance balances them and grows the forest on the device); without that flag it is refused with
// the way out.  --save_models keeps what self-training trained beside the forest (L95 and the Markov models: ml/model_bundle.hpp), and
// --model_file with --models_file scores with both, as the run that trained them did.  Deviations: INTEGRATION.md, "Known deviations".
#pragma once

#include <functional>
#include <string>

#include "junction_system.hpp"
#include "ml/model_features.hpp"
#include "prepared_files.hpp"

namespace portcullis {

struct JuncFilterException : public PortcullisException {
    explicit JuncFilterException(const std::string& m) : PortcullisException(m) {}
};

const std::string DEFAULT_FILTER_OUTPUT = "portcullis_filter/portcullis";
const std::string DEFAULT_FILTER_SOURCE = "portcullis";
const uint16_t DEFAULT_FILTER_THREADS = 1;
const double DEFAULT_FILTER_THRESHOLD = 0.5;

class JunctionFilter {
    std::string junctionFile;
    PreparedFiles prepData;
    std::string modelFile, modelsFile, filterFile, referenceFile, output;  // modelsFile: --models_file, the L95 and Markov models to score a saved forest with
    bool train = false;
    std::string selfTrainDir, trainingRule = "balanced";  // --self_train: the reference's data/ directory; a rule set in it (or a directory)
    bool smote = true, enn = false, saveLayers = false, saveMatrix = false;
    bool saveModels = false;  // --save_models: <output>.selftrain.models beside <output>.selftrain.forest
    uint16_t threads = DEFAULT_FILTER_THREADS;
    bool saveBad = false, saveFeatures = false, outputExonGFF = false, outputIntronGFF = false;
    uint32_t maxLength = 0, minCov = 1;
    bool filterCanonical = false, filterSemi = false, filterNovel = false;
    std::string source = DEFAULT_FILTER_SOURCE;
    double threshold = DEFAULT_FILTER_THRESHOLD;
    bool verbose = false;
    int device = 0;
    std::function<void()> beforeDevice;  // (setBeforeDevice)

    void forestPredict(const JunctionList& all, JunctionList& pass, JunctionList& fail, ml::ModelFeatures& mf, const ml::Forest& forest);
    // src/junction_filter.cc:278-437: true if a forest was trained (mf holds L95 and the Markov models, <output>.selftrain.forest is
    // written); false if the lenient rule file took its place (filterFile is set)
    bool selfTrain(const JunctionList& all, ml::ModelFeatures& mf, ml::Forest& forest);
    void printFilteringResults(const JunctionList& in, const JunctionList& pass, const JunctionList& fail, const std::string& prefix);

public:
    JunctionFilter(const std::string& prepDir, const std::string& junctionFile, const std::string& output)
        : junctionFile(junctionFile), prepData(prepDir), output(output) {}

    void setSaveBad(bool v) { saveBad = v; }
    void setSource(const std::string& v) { source = v; }
    void setVerbose(bool v) { verbose = v; }
    void setThreads(uint16_t v) { threads = v; }
    void setMaxLength(uint32_t v) { maxLength = v; }
    void setMinCov(uint32_t v) { minCov = v; }
    uint32_t getMinCov() const { return minCov; }
    void setCanonical(const std::string& canonical);  // "OFF", or up to two of C, S, N separated by commas: what to KEEP
    bool doCanonicalFiltering() const { return filterCanonical || filterSemi || filterNovel; }
    void setOutputExonGFF(bool v) { outputExonGFF = v; }
    void setOutputIntronGFF(bool v) { outputIntronGFF = v; }
    void setFilterFile(const std::string& v) { filterFile = v; }
    void setModelFile(const std::string& v) { modelFile = v; }
    void setModelsFile(const std::string& v) { modelsFile = v; }
    void setSaveModels(bool v) { saveModels = v; }
    void setReferenceFile(const std::string& v) { referenceFile = v; }
    void setTrain(bool v) { train = v; }
    void setSelfTrainDir(const std::string& v) { selfTrainDir = v; }
    void setTrainingRule(const std::string& v) { trainingRule = v; }
    void setSmote(bool v) { smote = v; }
    void setENN(bool v) { enn = v; }
    void setSaveLayers(bool v) { saveLayers = v; }
    void setSaveMatrix(bool v) { saveMatrix = v; }
    void setSaveFeatures(bool v) { saveFeatures = v; }
    void setThreshold(double v) { threshold = v; }
    void setDevice(int v) { device = v; }
    // Called once, right before filter() first touches the device (never on a route that needs none): a driver that ran another stage
    // on the device in this process waits here until that stage's memory is back.  Loading the table, the rule files and the initial
    // sets come before it.
    void setBeforeDevice(std::function<void()> f) { beforeDevice = std::move(f); }

    void filter();

    static std::string title() { return "Portcullis Filter Mode Help"; }
    static std::string description();
    static std::string usage() { return "portcullis_amd filt [options] <prep_data_dir> <junction_tab_file>"; }
    static std::string helpMessage();
    static int main(int argc, char* argv[]);
};

}  // namespace portcullis
