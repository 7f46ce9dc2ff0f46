// filt_parsers.cc -- the two host parsers of `filt` behind a main of their own (tests/test_host_filt.py; also what a sanitizer build runs:
// g++ -fsanitize=address,undefined -Iportcullis_amd/host/include tests/cpp/filt_parsers.cc portcullis_amd/host/src/forest.cc
// portcullis_amd/host/src/rule_filter.cc).
//   filt_parsers forest <file>          the arrays Forest::load makes of a ranger forest file, as text (doubles as hex floats)
//   filt_parsers rules <json> <tab>     one line of 0 / 1 per junction of the table: RuleFilter over its text
// A PortcullisException leaves with status 4 and its message on stderr, as the program does.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>

#include <portcullis/ml/forest.hpp>

#include "../../portcullis_amd/host/src/rule_filter.hpp"

template <typename T>
static void put(const char* name, const std::vector<T>& v) {
    std::cout << name;
    for (const auto& x : v) std::cout << " " << (long long)x;
    std::cout << "\n";
}
static void putd(const char* name, const std::vector<double>& v) {
    printf("%s", name);
    for (const double x : v) printf(" %a", x);
    printf("\n");
}

int main(int argc, char* argv[]) {
    try {
        if (argc == 3 && strcmp(argv[1], "forest") == 0) {
            const portcullis::ml::Forest f = portcullis::ml::Forest::load(argv[2]);
            std::cout << "header " << f.nTrees << " " << f.nVars << " " << f.dependentVar << "\n";
            put("is_ordered", f.isOrdered);
            std::cout.flush();
            putd("class_values", f.classValues);
            fflush(stdout);
            put("tree_off", f.treeOff);
            put("left", f.left);
            put("right", f.right);
            put("split_var", f.splitVar);
            put("count_off", f.countOff);
            std::cout.flush();
            putd("split_value", f.splitValue);
            putd("counts", f.counts);
            return 0;
        }
        if (argc == 4 && strcmp(argv[1], "rules") == 0) {
            portcullis::RuleFilter rules = portcullis::RuleFilter::load(argv[2]);
            std::ifstream in(argv[3]);
            std::string line;
            std::vector<std::string> fields;
            std::vector<std::vector<std::string>> rows;
            while (std::getline(in, line)) {
                if (line.empty()) continue;
                std::vector<std::string> cells(1);
                for (const char c : line) {
                    if (c == '\t') cells.emplace_back();
                    else cells.back().push_back(c);
                }
                cells.erase(cells.begin());  // the index column
                if (fields.empty()) fields = cells;
                else rows.push_back(cells);
            }
            for (const char p : rules.evaluate(fields, rows)) std::cout << (p ? '1' : '0');
            std::cout << "\n";
            return 0;
        }
    } catch (const portcullis::PortcullisException& e) {
        std::cerr << "Error: " << e.what() << std::endl;
        return 4;
    }
    std::cerr << "usage: filt_parsers forest <file> | rules <json> <tab>" << std::endl;
    return 1;
}
