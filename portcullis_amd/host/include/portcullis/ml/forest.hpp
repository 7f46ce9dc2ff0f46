// Forest: a saved ranger 0.3.8 probability forest (the .forest file a reference run leaves as <prefix>.selftrain.forest) as plain
// arrays -- what pjb_forest_check / pjb_forest_load take.  The layout read is that of Forest::saveToFile,
// ForestProbability::saveToFileInternal, Tree::appendToFile and TreeProbability::appendToFileInternal with the vector writers of
// utility.h:68-150 (little-endian; a vector is a u64 length and its elements, a 2-D vector a u64 length and that many vectors).
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "../bam/bam_master.hpp"

struct pjb_forest;

namespace portcullis {
namespace ml {

struct ForestException : public PortcullisException {
    explicit ForestException(const std::string& m) : PortcullisException(m) {}
};

struct Forest {
    int32_t nTrees = 0, nVars = 0, dependentVar = 0;
    std::vector<uint8_t> isOrdered;    // per variable
    std::vector<double> classValues;   // predictions come in this order
    std::vector<int64_t> treeOff;      // nTrees + 1: tree t owns the nodes treeOff[t] .. treeOff[t + 1]
    std::vector<int32_t> left, right;  // per node, inside the tree; -1 = no such child
    std::vector<int32_t> splitVar;
    std::vector<double> splitValue;
    std::vector<int64_t> countOff;     // per node: its class counts in `counts`, -1 = none
    std::vector<double> counts;

    // Throws ForestException for a file that cannot be opened, is not a probability forest, ends early or goes on after its last tree.
    static Forest load(const std::string& path);
    static Forest parse(const uint8_t* data, size_t size, const std::string& name);
    // The exact inverse of load / parse: the bytes Forest::saveToFile, ForestProbability::saveToFileInternal, Tree::appendToFile and
    // TreeProbability::appendToFileInternal write.  save throws ForestException for a file that cannot be written.
    std::vector<uint8_t> serialize() const;
    void save(const std::string& path) const;
    // a copy of the arrays the C ABI hands out (pjb_forest_grow's result) with their class values
    static Forest fromView(const pjb_forest& view, const double* classValues);
    // the view the C ABI takes (valid while this object lives and is not changed)
    void view(pjb_forest& out) const;
};

}  // namespace ml
}  // namespace portcullis
