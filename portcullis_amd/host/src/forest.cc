// Forest: see portcullis/ml/forest.hpp.  File layout: deps/ranger-0.3.8 of the reference (Forest::saveToFile and the writers it calls).
#include <portcullis/ml/forest.hpp>

#include <cstring>
#include <fstream>
#include <iterator>

#include "../../../include/portcullis_amd.h"

namespace portcullis {
namespace ml {

namespace {
struct Cursor {
    const uint8_t* p;
    size_t size, at = 0;
    const std::string& name;
    [[noreturn]] void truncated() const { throw ForestException("Forest model file ends inside the forest (truncated file): " + name); }
    template <typename T>
    T take() {
        if (size - at < sizeof(T)) truncated();
        T v;
        memcpy(&v, p + at, sizeof(T));
        at += sizeof(T);
        return v;
    }
    // a length that the rest of the file can hold, `each` bytes an element at least
    size_t length(size_t each) {
        const uint64_t n = take<uint64_t>();
        if (n > (size - at) / each) truncated();
        return (size_t)n;
    }
};
}  // namespace

Forest Forest::parse(const uint8_t* data, size_t size, const std::string& name) {
    Cursor c{data, size, 0, name};
    Forest f;
    const uint64_t dep = c.take<uint64_t>(), nTrees = c.take<uint64_t>();
    f.isOrdered.resize(c.length(1));
    for (auto& o : f.isOrdered) o = c.take<uint8_t>();
    const uint64_t nVars = c.take<uint64_t>();
    if (f.isOrdered.size() != nVars)
        throw ForestException("Forest model file: " + std::to_string(f.isOrdered.size()) + " ordered flags for " + std::to_string(nVars) + " variables: " + name);
    const int32_t treeType = c.take<int32_t>();
    if (treeType != 9) throw ForestException("Wrong treetype. Loaded file is not a probability estimation forest: " + name);
    f.classValues.resize(c.length(8));
    for (auto& v : f.classValues) v = c.take<double>();
    if (nTrees > 0x7fffffffull || nVars > 0x7fffffffull || dep > 0x7fffffffull || nTrees > size)
        throw ForestException("Forest model file holds counts no forest has: " + name);
    f.nTrees = (int32_t)nTrees;
    f.nVars = (int32_t)nVars;
    f.dependentVar = (int32_t)dep;
    f.treeOff.push_back(0);
    for (uint64_t t = 0; t < nTrees; t++) {
        const size_t nNodes = c.length(8);
        const size_t base = f.left.size();
        for (size_t k = 0; k < nNodes; k++) {  // child_nodeIDs: per node its children
            const size_t nc = c.length(8);
            int64_t ch[2] = {-1, -1};
            for (size_t i = 0; i < nc; i++) {
                const uint64_t id = c.take<uint64_t>();
                if (i < 2) ch[i] = id > 0x7ffffffeull ? 0x7fffffff : (int64_t)id;  // (a child outside the tree: pjb_forest_check says so)
            }
            if (nc > 2) throw ForestException("Forest model file: tree " + std::to_string(t) + ", node " + std::to_string(k) + " has " + std::to_string(nc) + " children: " + name);
            f.left.push_back((int32_t)ch[0]);
            f.right.push_back((int32_t)ch[1]);
        }
        const size_t nVar = c.length(8);
        if (nVar != nNodes) throw ForestException("Forest model file: tree " + std::to_string(t) + " has " + std::to_string(nNodes) + " nodes and " + std::to_string(nVar) + " split variables: " + name);
        for (size_t k = 0; k < nNodes; k++) {
            const uint64_t v = c.take<uint64_t>();
            f.splitVar.push_back(v > 0x7ffffffeull ? 0x7fffffff : (int32_t)v);
        }
        const size_t nVal = c.length(8);
        if (nVal != nNodes) throw ForestException("Forest model file: tree " + std::to_string(t) + " has " + std::to_string(nNodes) + " nodes and " + std::to_string(nVal) + " split values: " + name);
        for (size_t k = 0; k < nNodes; k++) f.splitValue.push_back(c.take<double>());
        f.countOff.resize(base + nNodes, -1);
        std::vector<uint64_t> terminal(c.length(8));
        for (auto& n : terminal) n = c.take<uint64_t>();
        const size_t nRows = c.length(8);
        if (nRows != terminal.size()) throw ForestException("Forest model file: tree " + std::to_string(t) + " lists " + std::to_string(terminal.size()) + " terminal nodes and " + std::to_string(nRows) + " rows of class counts: " + name);
        for (size_t i = 0; i < nRows; i++) {
            const size_t n = c.length(8);
            if (terminal[i] >= nNodes) throw ForestException("Forest model file: tree " + std::to_string(t) + " has class counts for node " + std::to_string(terminal[i]) + " of " + std::to_string(nNodes) + ": " + name);
            // (a row of another length than the class values: left without counts, pjb_forest_check names the node)
            if (n == f.classValues.size()) f.countOff[base + terminal[i]] = (int64_t)f.counts.size();
            for (size_t k = 0; k < n; k++) {
                const double v = c.take<double>();
                if (n == f.classValues.size()) f.counts.push_back(v);
            }
        }
        f.treeOff.push_back((int64_t)f.left.size());
    }
    if (c.at != size) throw ForestException("Forest model file goes on after its last tree (" + std::to_string(size - c.at) + " bytes too long): " + name);
    return f;
}

Forest Forest::load(const std::string& path) {
    std::ifstream in(path, std::ios::binary);
    if (!in.good()) throw ForestException("Could not read from input file: " + path + ".");
    const std::vector<char> raw((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    return parse((const uint8_t*)raw.data(), raw.size(), path);
}

std::vector<uint8_t> Forest::serialize() const {
    std::vector<uint8_t> out;
    auto put = [&out](const void* p, size_t n) { out.insert(out.end(), (const uint8_t*)p, (const uint8_t*)p + n); };
    auto u64 = [&put](uint64_t v) { put(&v, 8); };
    u64((uint64_t)dependentVar);
    u64((uint64_t)nTrees);
    u64(isOrdered.size());  // saveVector1D of a vector<bool>: the length, a byte an element
    put(isOrdered.data(), isOrdered.size());
    u64((uint64_t)nVars);
    const int32_t treeType = 9;  // TREE_PROBABILITY
    put(&treeType, 4);
    u64(classValues.size());
    put(classValues.data(), classValues.size() * 8);
    const size_t nClasses = classValues.size();
    for (int32_t t = 0; t < nTrees; t++) {
        const size_t a = (size_t)treeOff[(size_t)t], b = (size_t)treeOff[(size_t)t + 1];
        u64(b - a);  // child_nodeIDs: a vector per node, empty at a terminal node
        for (size_t k = a; k < b; k++) {
            const int nc = (left[k] >= 0) + (right[k] >= 0 && left[k] >= 0);
            u64((uint64_t)nc);
            if (nc > 0) u64((uint64_t)left[k]);
            if (nc > 1) u64((uint64_t)right[k]);
        }
        u64(b - a);
        for (size_t k = a; k < b; k++) u64((uint64_t)splitVar[k]);
        u64(b - a);
        put(splitValue.data() + a, (b - a) * 8);
        size_t terminal = 0;
        for (size_t k = a; k < b; k++) terminal += countOff[k] >= 0;
        u64(terminal);
        for (size_t k = a; k < b; k++)
            if (countOff[k] >= 0) u64(k - a);
        u64(terminal);
        for (size_t k = a; k < b; k++)
            if (countOff[k] >= 0) {
                u64(nClasses);
                put(counts.data() + countOff[k], nClasses * 8);
            }
    }
    return out;
}

void Forest::save(const std::string& path) const {
    const std::vector<uint8_t> raw = serialize();
    std::ofstream out(path, std::ios::binary);
    if (out.good()) out.write((const char*)raw.data(), (std::streamsize)raw.size());
    out.close();
    if (!out.good()) throw ForestException("Could not write to output file: " + path + ".");
}

Forest Forest::fromView(const pjb_forest& v, const double* classValues) {
    Forest f;
    f.nTrees = v.n_trees;
    f.nVars = v.n_vars;
    f.dependentVar = v.dependent_var;
    if (v.is_ordered) f.isOrdered.assign(v.is_ordered, v.is_ordered + v.n_vars);
    else f.isOrdered.assign((size_t)v.n_vars, 1);
    f.classValues.assign(classValues, classValues + v.n_classes);
    f.treeOff.assign(v.tree_off, v.tree_off + v.n_trees + 1);
    const size_t n = (size_t)f.treeOff.back();
    f.left.assign(v.left, v.left + n);
    f.right.assign(v.right, v.right + n);
    f.splitVar.assign(v.split_var, v.split_var + n);
    f.splitValue.assign(v.split_value, v.split_value + n);
    f.countOff.assign(v.count_off, v.count_off + n);
    f.counts.assign(v.counts, v.counts + v.n_counts);
    return f;
}

void Forest::view(pjb_forest& out) const {
    memset(&out, 0, sizeof out);
    out.n_trees = nTrees;
    out.n_classes = (int32_t)classValues.size();
    out.n_vars = nVars;
    out.dependent_var = dependentVar;
    out.is_ordered = isOrdered.data();
    out.tree_off = treeOff.data();
    out.left = left.data();
    out.right = right.data();
    out.split_var = splitVar.data();
    out.split_value = splitValue.data();
    out.count_off = countOff.data();
    out.counts = counts.data();
    out.n_counts = (int64_t)counts.size();
}

}  // namespace ml
}  // namespace portcullis
