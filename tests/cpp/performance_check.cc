// The host's Performance / PerformanceList (portcullis/ml/performance.hpp) from the command line: every argument is a confusion matrix
// "tp,tn,fp,fn"; prints each one's toLongString(), a line "--", then outputMeanPerformance over all of them.  No device, no library:
// tests/test_cv_model.py compiles this with src/performance.cc.
#include <portcullis/ml/performance.hpp>

#include <cstdio>
#include <iostream>
#include <memory>

int main(int argc, char* argv[]) {
    portcullis::ml::PerformanceList list;
    for (int i = 1; i < argc; i++) {
        unsigned tp, tn, fp, fn;
        if (sscanf(argv[i], "%u,%u,%u,%u", &tp, &tn, &fp, &fn) != 4) return 2;
        auto p = std::make_shared<portcullis::ml::Performance>(tp, tn, fp, fn);
        std::cout << p->toLongString() << "\n";
        list.add(p);
    }
    std::cout << "--\n";
    if (list.size()) list.outputMeanPerformance(std::cout);
    return 0;
}
