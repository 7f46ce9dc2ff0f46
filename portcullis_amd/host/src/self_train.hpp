// Self-training's host side (`filt --self_train`): everything JunctionFilter::filter and ModelFeatures::trainInstance of the reference do
// between "load the table" and "grow the forest", but the nearest-neighbour search (pjb_knn, on the device):
//   * findLayers: the layer files of a rule set (find_jsons / sort_jsons, src/junction_filter.cc:96-150);
//   * createTrainingSets: the initial positive and negative junctions (create_training_sets,
//     scripts/portcullis/portcullis/rule_filter.py:134-333) over the text of a junction table, through RuleFilter: no Python;
//   * smoteSynthesize: Smote::execute after its KNN (lib/src/smote.cc:52-68);
//   * undersample: the negative set cut down to the positive set's size (lib/src/model_features.cc:289-294);
//   * ennKeep: ENN::execute after its KNN (lib/src/enn.cc:53-73).
// The reference draws with std::mt19937(12345) through libstdc++ 11's distributions; those are restated here (selftrain::uniformInt,
// uniformReal) so that the draws do not change with the standard library this is built against.
#pragma once

#include <cstdint>
#include <random>
#include <string>
#include <vector>

#include <portcullis/bam/bam_master.hpp>

namespace portcullis {
namespace selftrain {

struct SelfTrainException : public PortcullisException {
    explicit SelfTrainException(const std::string& m) : PortcullisException(m) {}
};

const uint32_t SEED = 12345;

struct Layers {
    std::string ruleset;  // the directory that was read
    std::vector<std::string> pos, neg;  // paths, by layer number
};
// trainingRule: a directory if one exists by that name, else a name under dataDir.  Throws with the reference's messages for a
// directory that does not exist and for a rule set without positive or without negative layers.
Layers findLayers(const std::string& trainingRule, const std::string& dataDir);

struct TrainingSets {
    std::vector<size_t> pos, neg;  // rows of the table, ascending
    uint32_t L95 = 0;
    // what --save_layers writes: the rows every layer let through (pos) or took (neg), then the intron-size layer (pos: absent if the
    // set had 100 rows or fewer)
    std::vector<std::vector<size_t>> posLayers, negLayers;
    bool posSizeLayer = false;
    std::string log;  // the script's LAYER / PASS / FAIL lines
};
// fieldnames / rows: as RuleFilter::evaluate takes them (the table without its index column); needs the columns size and maxmmes.
TrainingSets createTrainingSets(const std::vector<std::string>& fieldnames, const std::vector<std::vector<std::string>>& rows,
                                const std::vector<std::string>& posLayerFiles, const std::vector<std::string>& negLayerFiles);

// uniform_int_distribution<T>(0, hi)(gen), hi < 2^32 - 1, and uniform_real_distribution<double>(0, 1)(gen) of libstdc++ 11
uint32_t uniformInt(std::mt19937& gen, uint32_t hi);
double uniformReal(std::mt19937& gen);

// KNN's rule for the k it really uses (lib/src/knn.cc:33-36; Smote and ENN repeat it)
inline int32_t effectiveK(size_t rows, int32_t defaultK) { return rows < (size_t)defaultK && rows < 100 ? (int32_t)rows : defaultK; }

// data: rows x cols; nn: rows x k (pjb_knn).  smoteness * rows synthetic rows, row-major, `smoteness` per row in row order.
std::vector<double> smoteSynthesize(const double* data, size_t rows, size_t cols, const uint32_t* nn, size_t k, uint32_t smoteness);
// The indices of 0..size-1 that survive `while (size > keep) erase(begin + uniform(0, size))`: the bound is inclusive, and a draw of
// `size` -- erase(end()) -- removes the last element, as libstdc++'s vector of shared_ptr does.
std::vector<size_t> undersample(size_t size, size_t keep);
// labels: 0 / 1 per row.  A row stays iff at least `threshold` of its k neighbours (itself among them) carry its label.
std::vector<char> ennKeep(const uint32_t* nn, size_t rows, size_t k, const std::vector<char>& labels, uint32_t threshold);

}  // namespace selftrain
}  // namespace portcullis
