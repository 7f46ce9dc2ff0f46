// JunctionFilter: see portcullis/junction_filter.hpp.  Line numbers refer to src/junction_filter.cc of the reference.
#include <portcullis/junction_filter.hpp>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iomanip>
#include <iostream>
#include <unordered_set>

#include "../../../include/portcullis_amd.h"
#include "fs_util.hpp"
#include "rule_filter.hpp"
#include "self_train.hpp"

using std::cout;
using std::endl;
using std::string;

namespace portcullis {

namespace {
std::vector<string> splitOn(const string& s, char sep, bool compress) {
    std::vector<string> parts(1);
    for (const char c : s) {
        if (c != sep) parts.back().push_back(c);
        else if (!compress || !parts.back().empty() || parts.size() == 1) parts.emplace_back();
    }
    return parts;
}
string trim(const string& s) {
    size_t a = 0, b = s.size();
    while (a < b && isspace((unsigned char)s[a])) a++;
    while (b > a && isspace((unsigned char)s[b - 1])) b--;
    return s.substr(a, b - a);
}
string locationAsString(const Junction& j) { return j.getIntron()->toString() + bam::strandToChar(j.getConsensusStrand()); }
}  // namespace

void JunctionFilter::setCanonical(const string& canonical) {  // junction_filter.hpp:277-307
    std::vector<string> modes;
    for (const string& m : splitOn(canonical, ',', true))
        if (!m.empty() || modes.empty()) modes.push_back(m);
    if (modes.size() > 3) throw JuncFilterException("Canonical filter mode contains too many modes.  Max is 2.");
    filterCanonical = filterSemi = filterNovel = true;
    for (string n : modes) {
        std::transform(n.begin(), n.end(), n.begin(), [](unsigned char c) { return (char)toupper(c); });
        if (n == "OFF") filterCanonical = filterSemi = filterNovel = false;
        else if (n == "C") filterCanonical = false;
        else if (n == "S") filterSemi = false;
        else if (n == "N") filterNovel = false;
    }
}

void JunctionFilter::printFilteringResults(const JunctionList& in, const JunctionList& pass, const JunctionList& fail, const string& prefix) {  // :607-620
    (void)fail;
    const size_t diff = in.size() - pass.size();
    cout << endl << prefix << endl << "-------------------------" << endl << "Input contained " << in.size() << " junctions." << endl
         << "Output contains " << pass.size() << " junctions." << endl << "Filtered out " << diff << " junctions." << endl;
}

void JunctionFilter::forestPredict(const JunctionList& all, JunctionList& pass, JunctionList& fail, ml::ModelFeatures& mf, const ml::Forest& forest) {  // :646-738
    cout << "Creating feature vector" << endl << "Initialising random forest" << endl << "Making predictions" << endl;
    std::vector<double> features;
    mf.setDevice(device);
    const std::vector<double> pred = mf.forestPredict(all, forest, saveFeatures || saveMatrix ? &features : nullptr);
    const size_t nClasses = forest.classValues.size();
    if (saveMatrix) {  // the 29 active columns of every junction as scored: little-endian f64, no header
        const std::vector<int32_t>& active = ml::ModelFeatures::activeFeatures();
        const size_t F = ml::ModelFeatures::featureNames().size();
        std::vector<double> m(all.size() * active.size());
        for (size_t i = 0; i < all.size(); i++)
            for (size_t k = 0; k < active.size(); k++) m[i * active.size() + k] = features[i * F + (size_t)active[k]];
        std::ofstream fout((output + ".testing.matrix.f64").c_str(), std::ios::binary);
        fout.write((const char*)m.data(), (std::streamsize)(m.size() * sizeof(double)));
    }
    if (saveFeatures) {  // :649-657: the active columns, default stream formatting
        std::ofstream fout((output + ".features.testing").c_str());
        const std::vector<string> names = ml::ModelFeatures::featureNames();
        const std::vector<int32_t>& active = ml::ModelFeatures::activeFeatures();
        fout << Intron::locationOutputHeader();
        for (const int32_t k : active) fout << "\t" << names[(size_t)k];
        fout << endl;
        for (size_t i = 0; i < all.size(); i++) {
            fout << *(all[i]->getIntron());
            for (const int32_t k : active) fout << "\t" << features[i * names.size() + (size_t)k];
            fout << endl;
        }
    }
    for (size_t i = 0; i < all.size(); i++) all[i]->setScore(1.0 - pred[i * nClasses]);  // 1 - P(class_values[0])
    cout << "Threshold set at " << threshold << endl;
    for (size_t i = 0; i < all.size(); i++) {  // categorise, :730-738
        if ((1.0 - pred[i * nClasses]) >= threshold) pass.push_back(all[i]);
        else fail.push_back(all[i]);
    }
}

namespace {
// the junctions as the table the rule engine reads: the columns but the index, one vector of cells per junction
void asTable(const JunctionList& juncs, std::vector<string>& fieldnames, std::vector<std::vector<string>>& table) {
    fieldnames = splitOn(Junction::junctionOutputHeader(), '\t', false);
    fieldnames.erase(fieldnames.begin());  // (the index column is the table's index, not a field)
    table.clear();
    table.reserve(juncs.size());
    string row;
    for (auto& j : juncs) {
        row.clear();
        j->appendTabRow(row);
        std::vector<string> cells = splitOn(row, '\t', false);
        cells.erase(cells.begin());
        table.push_back(std::move(cells));
    }
}
void saveTab(const string& path, const JunctionList& all, const std::vector<size_t>& rows) {
    std::ofstream out(path.c_str());
    out << Junction::junctionOutputHeader() << "\n";
    for (const size_t r : rows) out << *all[r] << "\n";
    if (!out.good()) throw JuncFilterException("Could not write " + path);
}
}  // namespace

bool JunctionFilter::selfTrain(const JunctionList& all, ml::ModelFeatures& mf, ml::Forest& forest) {  // :278-437
    const string lowJuncs = selfTrainDir + "/low_juncs_filter.json";
    if (all.size() < 200) {
        cout << "Less that 200 junctions found in input set.  This is not enough to build a trained model.  Will apply a lenient rule-based filter instead." << endl;
        filterFile = lowJuncs;
        return false;
    }
    if (all.size() < 500)  // rule_filter.py:142-143 raises here, and the reference dies of it
        throw JuncFilterException("Not enough junctions to create training set: self-training needs 500 junctions at least and the input holds " +
                                  std::to_string(all.size()) + " (the reference's script raises here and the reference ends).  With fewer than 200 a lenient rule file "
                                  "is applied instead; between the two, pass a model with --model_file, or --no_ml with --filter_file.");
    cout << "Self training mode activated." << endl << endl;
    const selftrain::Layers layers = selftrain::findLayers(trainingRule, selfTrainDir);
    cout << "Applying the following set of rule-based filters to create initial positive set." << endl;
    for (size_t i = 0; i < layers.pos.size(); i++) cout << i + 1 << "\t" << layers.pos[i] << endl;
    cout << "Applying a set of rule-based filters to create initial negative set." << endl;
    for (size_t i = 0; i < layers.neg.size(); i++) cout << i + 1 << "\t" << layers.neg[i] << endl;
    std::vector<string> fieldnames;
    std::vector<std::vector<string>> table;
    asTable(all, fieldnames, table);
    const selftrain::TrainingSets sets = selftrain::createTrainingSets(fieldnames, table, layers.pos, layers.neg);
    cout << sets.log << endl;
    const string prefix = output + ".selftrain.initialset";
    {
        std::ofstream l95out((prefix + ".L95_intron_size.txt").c_str());
        l95out << "Length of intron at 95th percentile" << "\n" << sets.L95 << "\n";
    }
    if (saveLayers) {
        for (size_t i = 0; i < sets.posLayers.size(); i++) {
            const bool sizeLayer = sets.posSizeLayer && i + 1 == sets.posLayers.size();
            saveTab(prefix + (sizeLayer ? string(".pos_layer_intronsize.tab") : ".pos_layer_" + std::to_string(i + 1) + ".tab"), all, sets.posLayers[i]);
        }
        for (size_t i = 0; i < sets.negLayers.size(); i++) {
            const bool sizeLayer = i + 1 == sets.negLayers.size();
            saveTab(prefix + (sizeLayer ? string(".neg_layer_intronsize.tab") : ".neg_layer_" + std::to_string(i + 1) + ".tab"), all, sets.negLayers[i]);
        }
    }
    saveTab(prefix + ".pos.junctions.tab", all, sets.pos);
    saveTab(prefix + ".neg.junctions.tab", all, sets.neg);
    JunctionList pos, neg;
    for (const size_t r : sets.pos) pos.push_back(all[r]);
    for (const size_t r : sets.neg) neg.push_back(all[r]);
    std::sort(pos.begin(), pos.end(), JunctionComparator());  // posSystem.sort() / negSystem.sort()
    std::sort(neg.begin(), neg.end(), JunctionComparator());
    cout << "Initial training set consists of " << pos.size() << " positive and " << neg.size() << " negative junctions." << endl << endl;
    if (pos.size() < 50 || neg.size() < 50) {
        cout << "Training set is of insufficient size to reliably use machine learning, we will filter junctions using a lenient rule-based filter instead." << endl;
        filterFile = lowJuncs;
        return false;
    }
    if (beforeDevice) beforeDevice();
    if (pjb_device_count() <= 0)
        throw JuncFilterException("No MI355X (HIP device) is visible: self-training searches neighbours and grows its forest on the GPU and has no CPU fallback.  "
                                  "Run filt where the GPU is.");
    // the reference's sets are junctions of their own, read back from the two tables; here they are the input's, and get their flags back
    std::vector<bool> genuineBefore;
    for (auto& j : all) genuineBefore.push_back(j->isGenuine());
    for (auto& j : pos) j->setGenuine(true);
    for (auto& j : neg) j->setGenuine(false);
    cout << "Pos to neg ratio: " << 1.0 - ((double)pos.size() / (double)(pos.size() + neg.size())) << endl << endl;
    mf.initGenomeMapper(prepData.getGenomeFilePath());
    mf.L95 = sets.L95;
    cout << "Confirming intron length L95 is: " << mf.L95 << endl;
    cout << "Feature learning from training set ...";
    cout.flush();
    mf.setDevice(device);
    {  // one context for the training and for trainInstance: the genomes of both sets' targets are uploaded once
        JunctionList both = pos;
        both.insert(both.end(), neg.begin(), neg.end());
        mf.openDevice(both);
    }
    mf.trainCodingPotentialModel(pos);
    mf.trainSplicingModels(pos, neg);
    cout << " done." << endl << endl;
    cout << "Training Random Forest" << endl << "----------------------" << endl << endl;
    ml::ModelFeatures::TrainOptions o;
    o.smote = smote;
    o.enn = enn;
    o.saveFeatures = saveFeatures;
    o.verbose = verbose;
    o.outputPrefix = output + ".selftrain";
    std::vector<double> matrix;
    mf.setDevice(device);
    forest = mf.trainInstance(pos, neg, o, saveMatrix ? &matrix : nullptr);
    for (size_t i = 0; i < all.size(); i++) all[i]->setGenuine(genuineBefore[i]);
    if (saveMatrix) {
        std::ofstream fout((output + ".selftrain.matrix.f64").c_str(), std::ios::binary);
        fout.write((const char*)matrix.data(), (std::streamsize)(matrix.size() * sizeof(double)));
    }
    forest.save(output + ".selftrain.forest");
    cout << "Saved forest to file " << output << ".selftrain.forest" << endl << endl;
    if (saveModels) {
        mf.bundle().save(output + ".selftrain.models");
        cout << "Saved L95 and Markov models to file " << output << ".selftrain.models" << endl << endl;
    }
    return true;
}

void JunctionFilter::filter() {  // :153-596
    size_t slash = output.find_last_of('/');
    string outputDir = slash == string::npos ? string(".") : output.substr(0, slash);
    const string outputPrefix = slash == string::npos ? output : output.substr(slash + 1);
    if (outputDir.empty()) outputDir = "/";
    if (train && selfTrainDir.empty())
        throw JuncFilterException("Self-training a random forest model is not the default of portcullis_amd filt.  Ask for it with --self_train <data_dir> (the "
                                  "directory of the rule sets), pass a saved model with --model_file (the <prefix>.selftrain.forest file a self-training run "
                                  "leaves), or filter with rules only: --no_ml with --filter_file.");
    if (train && !isDirectory(selfTrainDir)) throw JuncFilterException("Could not find the self-training data directory at: " + selfTrainDir);
    if (!exists(junctionFile)) throw JuncFilterException("Could not find junction file at: " + junctionFile);
    if (!exists(prepData.getGenomeFilePath())) throw JuncFilterException("Could not find prepared genome file at: " + prepData.getGenomeFilePath());
    if (!modelFile.empty() && !exists(modelFile)) throw JuncFilterException("Could not find filter model file at: " + modelFile);
    if (!modelsFile.empty() && !exists(modelsFile)) throw JuncFilterException("Could not find Markov model file at: " + modelsFile);
    if (!filterFile.empty() && !exists(filterFile)) throw JuncFilterException("Could not find filter configuration file at: " + filterFile);
    if (!referenceFile.empty() && !exists(referenceFile)) throw JuncFilterException("Could not find reference BED file at: " + referenceFile);
    if (!exists(outputDir)) {
        if (!createDirectories(outputDir)) throw JuncFilterException("Could not create output directory at: " + outputDir);
    } else if (!isDirectory(outputDir))
        throw JuncFilterException("File exists with name of suggested output directory: " + outputDir);
    ml::ModelBundle bundle;  // --models_file: read and checked on the host, before the table is loaded or a device looked for
    if (!modelsFile.empty()) bundle = ml::ModelBundle::load(modelsFile);
    cout << "Loading junctions from " << junctionFile << " ...";
    cout.flush();
    JunctionSystem originalJuncs(junctionFile);
    cout << " done." << endl << "Found " << originalJuncs.getJunctions().size() << " junctions." << endl << endl;
    JunctionList currentJuncs = originalJuncs.getJunctions();

    std::unordered_set<string> ref;
    if (!referenceFile.empty()) {  // :204-224
        cout << "Loading junctions from reference: " << referenceFile << " ...";
        cout.flush();
        std::ifstream ifs(referenceFile.c_str());
        string line;
        while (std::getline(ifs, line)) {
            const std::vector<string> parts = splitOn(trim(line), '\t', true);
            if (parts.size() == 12) {  // any other line is no entry
                const int end = std::stoi(parts[7]) - 1;  // BED to portcullis coordinates
                ref.insert(parts[0] + "(" + parts[6] + "," + std::to_string(end) + ")" + parts[5]);
            }
        }
        cout << " done." << endl << "Found " << ref.size() << " junctions in reference." << endl << endl;
    }

    JunctionSystem discardedJuncs;
    if (train) {  // :278-456
        ml::ModelFeatures mf;  // (the genome is opened only if a forest is trained)
        ml::Forest forest;
        if (selfTrain(currentJuncs, mf, forest)) {
            ml::ModelFeatures::checkForest(forest);
            cout << "Predicting valid junctions using random forest model" << endl << "----------------------------------------------------" << endl << endl;
            JunctionList passJuncs, failJuncs;
            forestPredict(currentJuncs, passJuncs, failJuncs, mf, forest);  // the same ModelFeatures: the trained models and L95 score every junction
            printFilteringResults(currentJuncs, passJuncs, failJuncs, "Random Forest filtering results");
            currentJuncs = passJuncs;
            for (auto& j : failJuncs) discardedJuncs.addJunction(j);
        } else if (!exists(filterFile))
            throw JuncFilterException("Could not find filter configuration file at: " + filterFile);
    }
    if (!modelFile.empty()) {  // :441-456
        const ml::Forest forest = ml::Forest::load(modelFile);  // (read and checked before the genome or a device is touched)
        ml::ModelFeatures::checkForest(forest);
        ml::ModelFeatures mf;  // L95 = 0, untrained Markov models: nothing was trained in this run ...
        if (!modelsFile.empty()) mf.setBundle(bundle);  // ... unless the run that trained the forest left them
        mf.initGenomeMapper(prepData.getGenomeFilePath());
        cout << "Predicting valid junctions using random forest model" << endl << "----------------------------------------------------" << endl << endl;
        JunctionList passJuncs, failJuncs;
        if (beforeDevice) beforeDevice();
        forestPredict(currentJuncs, passJuncs, failJuncs, mf, forest);
        printFilteringResults(currentJuncs, passJuncs, failJuncs, "Random Forest filtering results");
        currentJuncs = passJuncs;
        for (auto& j : failJuncs) discardedJuncs.addJunction(j);
    }

    if (currentJuncs.empty()) {
        cout << "WARNING: No junctions left from input.  Will not apply any further filters." << endl;
    } else {
        if (!filterFile.empty()) {  // :463-503, without the script and its intermediate files
            RuleFilter rules = RuleFilter::load(filterFile);
            std::vector<string> fieldnames = splitOn(Junction::junctionOutputHeader(), '\t', false);
            const size_t scoreAt = (size_t)(std::find(fieldnames.begin(), fieldnames.end(), "score") - fieldnames.begin());
            fieldnames.erase(fieldnames.begin());  // (the index column is the table's index, not a field)
            std::vector<std::vector<string>> table;
            table.reserve(currentJuncs.size());
            string row;
            for (auto& j : currentJuncs) {
                row.clear();
                j->appendTabRow(row);  // what the .rules_in table would hold
                std::vector<string> cells = splitOn(row, '\t', false);
                j->setScore(strtod(cells.at(scoreAt).c_str(), nullptr));  // the junctions come back from a table: the score as printed (the one value not read from one)
                cells.erase(cells.begin());
                table.push_back(std::move(cells));
            }
            const std::vector<char> passed = rules.evaluate(fieldnames, table);
            JunctionList passJuncs, failJuncs;
            for (size_t i = 0; i < currentJuncs.size(); i++) (passed[i] ? passJuncs : failJuncs).push_back(currentJuncs[i]);
            std::sort(passJuncs.begin(), passJuncs.end(), JunctionComparator());  // posSystem.sort() / negSystem.sort()
            std::sort(failJuncs.begin(), failJuncs.end(), JunctionComparator());
            currentJuncs = passJuncs;
            for (auto& j : failJuncs) discardedJuncs.addJunction(j);
        }
        if (currentJuncs.empty()) {
            cout << "WARNING: Rule-based filter discarded all junctions from input.  Will not apply any further filters." << endl;
        } else if (maxLength > 0 || doCanonicalFiltering() || minCov > 1) {  // :509-546
            JunctionList passJuncs, failJuncs;
            for (auto& j : currentJuncs) {
                bool pass = true;
                if (maxLength > 0 && j->getIntronSize() > maxLength) pass = false;
                if (pass && doCanonicalFiltering()) {
                    if (filterNovel && j->getSpliceSiteType() == CanonicalSS::NO) pass = false;
                    if (filterSemi && j->getSpliceSiteType() == CanonicalSS::SEMI_CANONICAL) pass = false;
                    if (filterCanonical && j->getSpliceSiteType() == CanonicalSS::CANONICAL) pass = false;
                }
                if (pass && getMinCov() > j->getNbSplicedAlignments()) pass = false;
                if (pass) passJuncs.push_back(j);
                else {
                    failJuncs.push_back(j);
                    discardedJuncs.addJunction(j);
                }
            }
            printFilteringResults(currentJuncs, passJuncs, failJuncs, "Post filtering (length and/or canonical) results");
            currentJuncs = passJuncs;
        }
    }
    cout << endl;
    JunctionSystem filteredJuncs, refKeptJuncs;
    if (currentJuncs.empty()) {
        cout << "WARNING: Filters discarded all junctions from input." << endl;
    } else {  // :555-580
        cout << "Recalculating junction grouping and distance stats based on new junction list that passed filters ...";
        cout.flush();
        for (auto& j : currentJuncs) filteredJuncs.addJunction(j);
        uint32_t inref = 0;
        if (!referenceFile.empty()) {
            for (auto& j : currentJuncs)
                if (ref.count(locationAsString(*j)) > 0) inref++;
            for (auto& j : discardedJuncs.getJunctions())
                if (ref.count(locationAsString(*j)) > 0) {
                    filteredJuncs.addJunction(j);
                    refKeptJuncs.addJunction(j);
                    inref++;
                }
        }
        filteredJuncs.calcJunctionStats();
        cout << " done." << endl << endl;
        if (!referenceFile.empty()) {
            cout << "Brought back " << refKeptJuncs.size() << " junctions that were discarded by filters but were present in reference file." << endl;
            cout << "Your sample contains " << inref << " / " << ref.size() << " (" << ((double)inref / (double)ref.size()) * 100.0
                 << "%) junctions from the reference." << endl << endl;
        }
    }
    printFilteringResults(originalJuncs.getJunctions(), filteredJuncs.getJunctions(), discardedJuncs.getJunctions(), "Overall results");
    cout << endl << "Saving junctions passing filter to disk:" << endl;
    filteredJuncs.saveAll(outputDir + "/" + outputPrefix + ".pass", source + "_pass", true, outputExonGFF, outputIntronGFF);
    if (saveBad) {
        cout << "Saving junctions failing filter to disk:" << endl;
        discardedJuncs.saveAll(outputDir + "/" + outputPrefix + ".fail", source + "_fail", true, outputExonGFF, outputIntronGFF);
        if (!referenceFile.empty()) {
            cout << "Saving junctions failing filters but present in reference:" << endl;
            refKeptJuncs.saveAll(outputDir + "/" + outputPrefix + ".ref", source + "_ref", true, outputExonGFF, outputIntronGFF);
        }
    }
}

string JunctionFilter::description() {
    return "Filters out junctions that are unlikely to be genuine or that have too little\n"
           "supporting evidence.  A saved random forest model (--model_file) scores every\n"
           "junction on the GPU; rule files (--filter_file), the length, canonical and\n"
           "coverage filters and a reference annotation apply after it.  --self_train trains\n"
           "the model on the input itself (layered rule sets choose the initial junctions; the\n"
           "nearest-neighbour search and the forest run on the GPU); without it pass\n"
           "--model_file, or --no_ml with --filter_file.";
}

string JunctionFilter::helpMessage() {
    return title() + "\n\n" + description() + "\n\nUsage: " + usage() + "\n\n" +
           "System options:\n"
           "  -t [ --threads ] arg (=1)            Accepted for compatibility (the forest is walked on the GPU)\n"
           "  --devices arg                        Number of GPUs offered; the forest stage uses the first (no GPU is opened without a model)\n"
           "  -v [ --verbose ]                     Print extra information\n"
           "  --help                               Produce help message\n\n"
           "Output options:\n"
           "  -o [ --output ] arg (=" + DEFAULT_FILTER_OUTPUT + ")\n"
           "                                       Output prefix for files generated by this program.\n"
           "  -b [ --save_bad ]                    Saves bad junctions (i.e. junctions that fail the filter), as well as good junctions (those that pass)\n"
           "  --exon_gff                           Output exon-based junctions in GFF format.\n"
           "  --intron_gff                         Output intron-based junctions in GFF format.\n"
           "  --source arg (=" + DEFAULT_FILTER_SOURCE + ")            The value to enter into the \"source\" field in GFF files.\n\n"
           "Filtering options:\n"
           "  -f [ --filter_file ] arg             Rule-based filtering: a JSON file with the rules to apply (parameters and expression).\n"
           "  -r [ --reference ] arg               Reference annotation of junctions in BED format.  Junctions found in it are kept regardless of any other filter.\n"
           "  -n [ --no_ml ]                       Disables machine learning filtering\n"
           "  -m [ --model_file ] arg              A saved random forest model (a .forest file, e.g. <prefix>.selftrain.forest of a reference run) to score the junctions with.\n"
           "  --max_length arg (=0)                Filter junctions longer than this value.  Default (0) is to not filter based on length.\n"
           "  --canonical arg (=OFF)               Keep junctions based on their splice site status.  Valid options: OFF,C,S,N.  User can separate options by a comma to keep two categories.\n"
           "  --min_cov arg (=1)                   Only keep junctions with a number of split reads greater than or equal to this number\n"
           "  --models_file arg                    With --model_file: the L95 and Markov models to score with (<prefix>.selftrain.models of a --save_models run,\n"
           "                                       or <prefix>.models of train --markov).  Without it a saved forest is applied with L95 = 0 and untrained models.\n"
           "  --threshold arg (=0.5)               The threshold score at which we determine a junction to be genuine or not.\n"
           "  --save_features                      Save the feature rows of all junctions to <output>.features.testing\n\n"
           "Self-training options (refused without --self_train):\n"
           "  --self_train arg                     Train the model on the input: arg is the directory of the rule sets (laid out as the reference's data/:\n"
           "                                       <ruleset>/selftrain_initial_{pos,neg}.layerN.json and low_juncs_filter.json).  Not with --no_ml or --model_file.\n"
           "                                       Fewer than 200 junctions: low_juncs_filter.json is applied instead; 200 to 499: refused.\n"
           "  --training_rule arg (=balanced)      The rule set of the initial sets: a directory, or a name under the --self_train directory (balanced, precise).\n"
           "  --no_smote                           Disable the balancing of the two sets (synthetic oversampling, or under-sampling)\n"
           "  --enn                                Enable Edited Nearest Neighbour to clean the decision region\n"
           "  --save_layers                        Save each layer produced when creating the training set\n"
           "  --save_models                        Save <output>.selftrain.models: the L95 and the Markov models the forest's rows were made with (for --models_file)\n"
           "  --save_matrix                        Save <output>.selftrain.matrix.f64 (the training matrix, rows x 29) and <output>.testing.matrix.f64\n"
           "                                       (the 29 columns of every junction as scored): little-endian doubles, no header\n\n"
           "Not built (refused): self-training without --self_train (neither --model_file nor --no_ml), -g [ --genuine ]\n";
}

int JunctionFilter::main(int argc, char* argv[]) {
    std::vector<string> positional;
    string output = DEFAULT_FILTER_OUTPUT, source = DEFAULT_FILTER_SOURCE, filterFile, referenceFile, modelFile, canonical = "OFF";
    string selfTrainDir, trainingRule = "balanced", modelsFile;
    bool saveBad = false, exongff = false, introngff = false, noMl = false, saveFeatures = false, verbose = false, help = false;
    bool noSmote = false, enn = false, saveLayers = false, saveMatrix = false, saveModels = false;
    std::vector<std::pair<string, string>> selfTrainOnly;  // the options that belong to self-training, as given: refused without --self_train
    int threads = DEFAULT_FILTER_THREADS;
    uint32_t maxLength = 0, minCov = 1;
    double threshold = DEFAULT_FILTER_THRESHOLD;
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
            if (i + 1 >= argc) throw JuncFilterException("Option " + a + " needs a value");
            return argv[++i];
        };
        auto notBuilt = [&](const string& what, const string& wayOut) {
            throw JuncFilterException(what + " is not built into portcullis_amd filt.  " + wayOut);
        };
        const string selfTrainOut = "It belongs to self-training; pass a saved model with --model_file, or --no_ml with --filter_file.";
        if (a == "-o" || a == "--output") output = need();
        else if (a == "-b" || a == "--save_bad") saveBad = true;
        else if (a == "--exon_gff") exongff = true;
        else if (a == "--intron_gff") introngff = true;
        else if (a == "--source") source = need();
        else if (a == "-f" || a == "--filter_file") filterFile = need();
        else if (a == "-r" || a == "--reference") referenceFile = need();
        else if (a == "-n" || a == "--no_ml") noMl = true;
        else if (a == "-m" || a == "--model_file") modelFile = need();
        else if (a == "--models_file") modelsFile = need();
        else if (a == "--max_length") maxLength = (uint32_t)std::stoul(need());
        else if (a == "--canonical") canonical = need();
        else if (a == "--min_cov") minCov = (uint32_t)std::stoul(need());
        else if (a == "--threshold") threshold = std::stod(need());
        else if (a == "--save_features") saveFeatures = true;
        else if (a == "-t" || a == "--threads") threads = std::stoi(need());
        else if (a == "--devices") (void)need();
        else if (a == "-v" || a == "--verbose") verbose = true;
        else if (a == "--help") help = true;
        else if (a == "--self_train") selfTrainDir = need();
        else if (a == "--training_rule") {
            trainingRule = need();
            selfTrainOnly.emplace_back("--training_rule (the rule sets of the self-training's initial layers)", selfTrainOut);
        } else if (a == "--no_smote") {
            noSmote = true;
            selfTrainOnly.emplace_back("--no_smote (synthetic oversampling of the training set)", selfTrainOut);
        } else if (a == "--enn") {
            enn = true;
            selfTrainOnly.emplace_back("--enn (Edited Nearest Neighbour cleaning of the training set)", selfTrainOut);
        } else if (a == "--save_layers") {
            saveLayers = true;
            selfTrainOnly.emplace_back("--save_layers (the layers of the training set)", selfTrainOut);
        } else if (a == "--save_models") {
            saveModels = true;
            selfTrainOnly.emplace_back("--save_models (the L95 and the Markov models self-training trains)", selfTrainOut);
        } else if (a == "--save_matrix") {
            saveMatrix = true;
            selfTrainOnly.emplace_back("--save_matrix (the training and the testing matrix of self-training)", selfTrainOut);
        }
        else if (a == "-g" || a == "--genuine")
            notBuilt("--genuine (performance tables against a list of known labels)", "Run without it; the .pass and .fail tables can be compared with the labels afterwards.");
        else if (!a.empty() && a[0] == '-' && a.size() > 1) throw JuncFilterException("Unknown option: " + a);
        else positional.push_back(a);
    }
    if (help || argc <= 1 || positional.size() < 2) {
        cout << helpMessage() << endl;
        return 1;
    }
    if (selfTrainDir.empty() && !selfTrainOnly.empty())
        throw JuncFilterException(selfTrainOnly[0].first + " is not built into portcullis_amd filt without --self_train <data_dir>.  " + selfTrainOnly[0].second);
    if (!selfTrainDir.empty() && (noMl || !modelFile.empty()))
        throw JuncFilterException("--self_train trains the model on the input: it cannot be combined with --no_ml or --model_file.");
    if (!modelsFile.empty() && (!selfTrainDir.empty() || noMl || modelFile.empty()))
        throw JuncFilterException("--models_file " + modelsFile + " holds the L95 and the Markov models a saved forest is scored with: it needs --model_file and cannot be "
                                  "combined with --self_train (which trains its own) or --no_ml.");
    const auto t0 = std::chrono::steady_clock::now();
    cout << "Running portcullis in junction filter mode" << endl << "------------------------------------------" << endl << endl;
    JunctionFilter filter(positional[0], positional[1], output);
    filter.setSaveBad(saveBad);
    filter.setSource(source);
    filter.setVerbose(verbose);
    filter.setThreads((uint16_t)std::max(1, threads));
    filter.setMaxLength(maxLength);
    filter.setCanonical(canonical);
    filter.setMinCov(minCov);
    filter.setOutputExonGFF(exongff);
    filter.setOutputIntronGFF(introngff);
    filter.setFilterFile(filterFile);
    if (modelFile.empty() && !noMl) filter.setTrain(true);  // the reference's default: refused by filter()
    else {
        filter.setTrain(false);
        if (!noMl) filter.setModelFile(modelFile);
        filter.setModelsFile(modelsFile);
    }
    filter.setSelfTrainDir(selfTrainDir);
    filter.setTrainingRule(trainingRule);
    filter.setSmote(!noSmote);
    filter.setENN(enn);
    filter.setSaveLayers(saveLayers);
    filter.setSaveMatrix(saveMatrix);
    filter.setSaveModels(saveModels);
    filter.setSaveFeatures(saveFeatures);
    filter.setReferenceFile(referenceFile);
    filter.setThreshold(threshold);
    filter.filter();
    const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    std::ios::fmtflags f(cout.flags());
    cout << endl << "Portcullis junction filter completed." << endl << "Total runtime: " << std::fixed << std::setprecision(1) << s << "s" << endl << endl;
    cout.flags(f);
    return 0;
}

}  // namespace portcullis
