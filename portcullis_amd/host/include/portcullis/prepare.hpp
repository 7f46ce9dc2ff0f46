// Prepare: `portcullis_amd prep` -- the prepared directory `junc` starts from (the class surface of the reference's
// src/prepare.hpp:147-230 and src/prepare.cc:89-332, 373-): the genome and its .fai, the coordinate-sorted BAM and its .bai,
// linked or copied under the names of PreparedFiles.  Where the reference shells out to `samtools index`
// (Prepare::bamIndex, src/prepare.cc:227-260) the index is built on the device: pjb_index_begin / _piece / _end over the
// file's BGZF blocks, read through a ring of page-locked pieces.  With --merge several coordinate-sorted BAM files are merged into
// the directory's one on the device (bamMerge, src/prepare.cc:154-195: pjb_bam_merge_*, a target at a time); without the flag a
// second file is refused.  With --sort a file the index build finds unsorted is sorted on the device (bamSort, src/prepare.cc:140-153:
// pjb_bam_sort_*, a run of the file at a time; several runs go through the merge); without the flag it is refused.  With --build_csi
// every index prep builds is a CSI (pjb_index_begin_csi / _end_csi: the depth htslib would choose), which also covers targets of 2^29
// bases or more; --use_csi without that flag stays refused, with a message that says what to do instead.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "prepared_files.hpp"

namespace portcullis {

const std::string DEFAULT_PREP_OUTPUT_DIR = "portcullis_prep";  // src/prepare.hpp:59
const uint16_t DEFAULT_PREP_THREADS = 1;

class Prepare {
    PreparedFiles output;
    bool force = false;
    bool useLinks = true;
    uint16_t threads = DEFAULT_PREP_THREADS;
    bool useCsi = false;
    bool buildCsi = false;
    bool verbose = false;
    bool merge = false;
    bool sort = false;

    // link or copy `from` to `to` unless `to` is there already (src/prepare.cc:98-128); true if `to` exists afterwards
    bool copy(const std::string& from, const std::string& to, const std::string& msg, bool requireInputFileExists);
    bool genomeIndex();
    bool bamIndex(bool indexCopied);
    void buildIndexOnDevice(const std::string& bamFile, const std::string& baiFile);
    // --merge: the header of the merged file (the inputs' headers checked against each other: portcullis/merge_header.hpp), and the
    // merge itself -- every input's share of a target through pjb_bam_merge_*, target after target, then the unplaced tails
    std::string mergedHeaderText(const std::vector<std::string>& bamFiles);
    void mergeBams(const std::vector<std::string>& bamFiles, const std::string& headerText);
    // --sort: `bamFile`, found unsorted, becomes the directory's sorted BAM: one read through the index build's piece reader feeds
    // pjb_bam_sort_*; one run is renamed into place, several (sortrunN.bam) are merged by mergeBams.  Files still to be removed when the
    // call returns or throws are added to tempPaths
    void sortBam(const std::string& bamFile, std::vector<std::string>& tempPaths);

public:
    explicit Prepare(const std::string& outputDir);

    void setForce(bool v) { force = v; }
    void setUseLinks(bool v) { useLinks = v; }
    void setUseCsi(bool v) { useCsi = v; }
    void setBuildCsi(bool v) { buildCsi = v; }
    void setThreads(uint16_t v) { threads = v; }
    void setVerbose(bool v) { verbose = v; }
    void setMerge(bool v) { merge = v; }
    void setSort(bool v) { sort = v; }
    const PreparedFiles& getOutput() const { return output; }

    // removes what a previous run left in the directory (PreparedFiles::clean, src/prepare.cc:77-86)
    void clean();
    void prepare(const std::vector<std::string>& bamFiles, const std::string& genomeFile);

    static std::string title() { return "Portcullis Prepare Mode Help"; }
    static std::string description() {
        return "Prepares a genome and a coordinate-sorted BAM file for the junction analysis: links (or copies) both into the\n"
               "output directory and indexes them.  A BAM index that is missing is built on the GPU (a BAI, or with --build_csi a CSI,\n"
               "which also covers targets of 2^29 bases or more).  With --merge several\n"
               "coordinate-sorted BAM files are merged into one on the GPU first; with --sort a BAM file that is not in coordinate\n"
               "order is sorted on the GPU.";
    }
    static std::string usage() { return "portcullis_amd prep [options] <genome-file> <bam-file>"; }
    static int main(int argc, char* argv[]);
};

}  // namespace portcullis
