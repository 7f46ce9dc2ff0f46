// Full: the `full` mode -- prep, junc, filt (self-trained) and, with -b, bamfilt as one pipeline in one process (mainFull,
// src/portcullis.cc:164-394 of the reference): the same directory layout (<out>/1-prep, <out>/2-junc/portcullis_all.*,
// <out>/3-filt/portcullis_filtered.*, <out>/portcullis.filtered.bam), the same setters on the same four classes, the same banners.  filt
// reads junc's table back from the file, as the reference does, so the directory holds what the four commands run one after another leave.
// What a single process adds: one stage's working set on the device at a time.  junc takes its contexts and page-locked rings down on
// threads this driver owns (JuncTeardown), and filt waits for them where it first needs the device (JunctionFilter::setBeforeDevice):
// loading the table, the rule files and the initial sets run beside the teardown.  The other stages release what they hold before they
// return.  Two options are this program's own: --self_train <data_dir> (required: no data directory is shipped) and --devices.
#pragma once

#include <string>

#include "bam/bam_master.hpp"

namespace portcullis {

struct FullException : public PortcullisException {
    explicit FullException(const std::string& m) : PortcullisException(m) {}
};

const std::string DEFAULT_FULL_OUTPUT = "portcullis_out";  // src/portcullis.cc:205

class Full {
public:
    static std::string title() { return "Portcullis Full Pipeline Mode Help"; }
    static std::string description() {
        return "Runs prep, junc, filter, and optionally bamfilt, as a complete pipeline.  Assumes\n"
               "that the self-trained machine learning approach for filtering is to be used.";
    }
    static std::string usage() { return "portcullis_amd full [options] --self_train <data_dir> <genome-file> <bam-file>"; }
    static std::string helpMessage();
    static int main(int argc, char* argv[]);
};

}  // namespace portcullis
