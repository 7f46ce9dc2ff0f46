// forest_roundtrip <in.forest> <out.forest>: ml::Forest::load, then ml::Forest::save (tests/test_host_forest_save.py compares the files).
// Prints the forest's shape; exit status 3 with the message for a ForestException.
#include <portcullis/ml/forest.hpp>

#include <cstdio>

int main(int argc, char* argv[]) {
    if (argc != 3) {
        fprintf(stderr, "usage: forest_roundtrip <in.forest> <out.forest>\n");
        return 1;
    }
    try {
        const portcullis::ml::Forest f = portcullis::ml::Forest::load(argv[1]);
        f.save(argv[2]);
        printf("trees %d vars %d classes %zu nodes %lld bytes %zu\n", f.nTrees, f.nVars, f.classValues.size(), (long long)f.treeOff.back(), f.serialize().size());
    } catch (const portcullis::ml::ForestException& e) {
        fprintf(stderr, "%s\n", e.what());
        return 3;
    }
    return 0;
}
