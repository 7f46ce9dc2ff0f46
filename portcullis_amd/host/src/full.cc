// Full: see portcullis/full.hpp.  Line numbers refer to src/portcullis.cc of the reference.
#include <portcullis/bam_filter.hpp>
#include <portcullis/full.hpp>
#include <portcullis/junction_builder.hpp>
#include <portcullis/junction_filter.hpp>
#include <portcullis/prepare.hpp>

#include <algorithm>
#include <cstdio>
#include <iostream>
#include <memory>
#include <vector>

#include "fs_util.hpp"
#include "host_profile.hpp"
#include "self_train.hpp"

using std::cout;
using std::endl;
using std::string;

namespace portcullis {

string Full::helpMessage() {
    return title() + "\n\n" + description() + "\n\nUsage: " + usage() + "\n\n" +
           "System options:\n"
           "  -t [ --threads ] arg (=1)        The number of threads to use.  Note that increasing the number of threads will also increase memory requirements.  Default: 1\n"
           "  --devices arg                    Number of GPUs offered to junc and filt (default: all visible)\n"
           "  --device_mem arg                 Device memory junc may hold on one GPU: an integer with an optional K, M or G, as junc --device_mem (default: no budget)\n"
           "  -v [ --verbose ]                 Print extra information\n"
           "  --help                           Produce help message\n\n"
           "Output options:\n"
           "  -o [ --output ] arg (=" + DEFAULT_FULL_OUTPUT + ")\n"
           "                                   Output directory. Default: " + DEFAULT_FULL_OUTPUT + "\n"
           "  -b [ --bam_filter ]              Filter out alignments corresponding with false junctions.  Warning: this is time consuming; make sure you really want to do this first!\n"
           "  --exon_gff                       Output exon-based junctions in GFF format.\n"
           "  --intron_gff                     Output intron-based junctions in GFF format.\n"
           "  --source arg (=portcullis)       The value to enter into the \"source\" field in GFF files.\n\n"
           "Input options:\n"
           "  --force                          Whether or not to clean the output directory before processing, thereby forcing full preparation of the genome and bam files.  By default portcullis will only do what it thinks it needs to.\n"
           "  --copy                           Whether to copy files from input data to prepared data where possible, otherwise will use symlinks.  Will require more time and disk space to prepare input but is potentially more robust.\n"
           "  --keep_temp                      Whether keep any temporary files created during the prepare stage of portcullis.  This might include BAM files and indexes.\n"
           "  --use_csi                        Whether to use CSI indexing rather than BAI indexing (refused without --build_csi; with it, the same as --build_csi).\n"
           "  --build_csi                      The prepare stage builds CSI indexes on the GPU, as prep --build_csi does (also for targets of 2^29 bases or more, which a BAI cannot index), and the later stages read and write CSI.\n"
           "  --merge                          Several coordinate-sorted BAM files may follow the genome: the prepare stage merges them into one on the GPU, as prep --merge does (ties in position go to the file given first).  Without it a second BAM file is refused.\n"
           "  --sort                           A BAM file that is not in coordinate order is sorted on the GPU by the prepare stage, as prep --sort does (stable by target and position, unplaced records last).  Without it such a file is refused.\n\n"
           "Analysis options:\n"
           "  --orientation arg (=UNKNOWN)     The orientation of the reads that produced the BAM alignments: \"F\" (Single-end forward orientation); \"R\" (single-end reverse orientation); \"FR\" (paired-end, with reads sequenced towards center of fragment -> <-.  This is usual setting for most Illumina paired end sequencing); \"RF\" (paired-end, reads sequenced away from center of fragment <- ->); \"FF\" (paired-end, reads both sequenced in forward orientation); \"RR\" (paired-end, reads both sequenced in reverse orientation); \"UNKNOWN\" (default, portcullis will workaround any calculations requiring orientation information)\n"
           "  --strandedness arg (=UNKNOWN)    Whether BAM alignments were generated using a type of strand specific RNAseq library: \"unstranded\" (Standard Illumina); \"firststrand\" (dUTP, NSR, NNSR); \"secondstrand\" (Ligation, Standard SOLiD, flux sim reads); \"UNKNOWN\" (default, portcullis will workaround any calculations requiring strandedness information)\n"
           "  --separate                       Separate spliced from unspliced reads.\n"
           "  --extra                          Calculate additional metrics that take some time to generate.  (The reference re-reads the split files and so activates --separate; here the metrics come from the records in device memory, as in junc --extra.)\n\n"
           "Filtering options:\n"
           "  --self_train arg                 Required: the directory of the self-training rule sets (laid out as the reference's data/: <ruleset>/selftrain_initial_{pos,neg}.layerN.json and low_juncs_filter.json), as in filt --self_train.  No data directory is shipped with this program.\n"
           "  -r [ --reference ] arg           Reference annotation of junctions in BED format.  Any junctions found by the junction analysis tool will be preserved if found in this reference file regardless of any other filtering criteria.  If you need to convert a reference annotation from GTF or GFF to BED format portcullis contains scripts for this.\n"
           "  --max_length arg (=0)            Filter junctions longer than this value.  Default (0) is to not filter based on length.\n"
           "  --canonical arg (=OFF)           Keep junctions based on their splice site status.  Valid options: OFF,C,S,N. Where C = Canonical junctions (GT-AG), S = Semi-canonical junctions (AT-AC, or  GC-AG), N = Non-canonical.  OFF means, keep all junctions (i.e. don't filter by canonical status).  User can separate options by a comma to keep two categories.\n"
           "  --min_cov arg (=1)               Only keep junctions with a number of split reads greater than or equal to this number\n"
           "  --save_bad                       Saves bad junctions (i.e. junctions that fail the filter), as well as good junctions (those that pass)\n"
           "  --save_models                    Also save 3-filt/portcullis_filtered.selftrain.models: the L95 and the Markov models self-training trains, as filt --save_models\n"
           "  --training_rule arg (=balanced)  Pre-set to use for the self-training. Currently supported: balanced, precise. Default: balanced.\n\n"
           "Not built (refused, as in prep and filt): --genuine, a default data directory\n";
}

namespace {
void banner(const string& text) { cout << text << endl << string(text.size(), '-') << endl << endl; }
}  // namespace

int Full::main(int argc, char* argv[]) {
    std::vector<string> positional;
    string outputDir = DEFAULT_FULL_OUTPUT, referenceFile, strand = "UNKNOWN", ori = "UNKNOWN", source = "portcullis", canonical = "OFF";
    string selfTrainDir, trainingRule = "balanced";
    int threads = 1, devices = 0;
    uint64_t deviceMem = 0;
    bool separate = false, extra = false, copy = false, keepTemp = false, force = false, useCsi = false, buildCsi = false, merge = false, sort = false, saveBad = false, exongff = false,
         introngff = false, bamFilter = false, saveLayers = false, saveFeatures = false, saveModels = false, verbose = false, help = false;
    uint32_t maxLength = 0, minCov = 1;
    // long options take their value as the next argument or after '=' (as in filt)
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
            if (i + 1 >= argc) throw FullException("Option " + a + " needs a value");
            return argv[++i];
        };
        if (a == "-t" || a == "--threads") threads = std::stoi(need());
        else if (a == "--devices") devices = std::stoi(need());
        else if (a == "--device_mem") deviceMem = JunctionBuilder::parseDeviceMem(need());
        else if (a == "-v" || a == "--verbose") verbose = true;
        else if (a == "--help") help = true;
        else if (a == "-o" || a == "--output") outputDir = need();
        else if (a == "-b" || a == "--bam_filter") bamFilter = true;
        else if (a == "--exon_gff") exongff = true;
        else if (a == "--intron_gff") introngff = true;
        else if (a == "--source") source = need();
        else if (a == "--force") force = true;
        else if (a == "--copy") copy = true;
        else if (a == "--keep_temp") keepTemp = true;
        else if (a == "--use_csi") useCsi = true;
        else if (a == "--build_csi") buildCsi = true;
        else if (a == "--merge") merge = true;
        else if (a == "--sort") sort = true;
        else if (a == "--orientation") ori = need();
        else if (a == "--strandedness") strand = need();
        else if (a == "--separate") separate = true;
        else if (a == "--extra") extra = true;
        else if (a == "-r" || a == "--reference") referenceFile = need();
        else if (a == "--max_length") maxLength = (uint32_t)std::stoul(need());
        else if (a == "--canonical") canonical = need();
        else if (a == "--min_cov") minCov = (uint32_t)std::stoul(need());
        else if (a == "--save_bad") saveBad = true;
        else if (a == "--training_rule") trainingRule = need();
        else if (a == "--self_train") selfTrainDir = need();
        else if (a == "--save_features") saveFeatures = true;  // (hidden, as in the reference)
        else if (a == "--save_layers") saveLayers = true;      // (hidden, as in the reference)
        else if (a == "--save_models") saveModels = true;
        else if (!a.empty() && a[0] == '-' && a.size() > 1) throw FullException("Unknown option: " + a);
        else positional.push_back(a);
    }
    if (help || argc <= 1) {  // :282-288
        cout << helpMessage() << endl;
        return 1;
    }
    // everything that can be refused from the command line alone is refused before a file is touched or a device opened
    if (selfTrainDir.empty())
        throw FullException("portcullis_amd full needs --self_train <data_dir>: the directory of the self-training rule sets (the reference finds data/ beside "
                            "its program; this one ships none).  It has the meaning it has in filt --self_train.");
    if (positional.empty()) throw FullException("No genome file was given.  Usage: " + usage());
    if (positional.size() < 2) throw FullException("No BAM file was given.  Usage: " + usage());
    const string genomeFile = positional[0];
    const std::vector<string> bamFiles(positional.begin() + 1, positional.end());
    const bam::Orientation orientation = bam::orientationFromString(ori);
    const bam::Strandedness strandedness = bam::strandednessFromString(strand);
    struct stat st;
    if (lstat(genomeFile.c_str(), &st) != 0) throw FullException("Could not find genome file at: " + genomeFile);  // :298-301
    // filt's own checks of its self-training inputs, with filt's messages, before the stages that come before it have run
    if (!isDirectory(selfTrainDir)) throw JuncFilterException("Could not find the self-training data directory at: " + selfTrainDir);
    (void)selftrain::findLayers(trainingRule, selfTrainDir);
    if (!referenceFile.empty() && !exists(referenceFile)) throw JuncFilterException("Could not find reference BED file at: " + referenceFile);

    const bool prof = getenv("PJB_PROFILE_HOST") != nullptr;
    const double t0 = HostProfile::now();
    banner("Running full portcullis pipeline");
    if (!exists(outputDir) && !createDirectories(outputDir)) throw FullException("Could not create output directory: " + outputDir);

    // ---- 1-prep (:314-327).  Its index context and page-locked pieces are gone when prepare() returns.
    banner("Preparing input data (BAMs + genome)");
    const string prepDir = outputDir + "/1-prep";
    Prepare prep(prepDir);
    prep.setForce(force);
    prep.setUseLinks(!copy);
    prep.setUseCsi(useCsi);
    prep.setBuildCsi(buildCsi);
    prep.setMerge(merge);
    prep.setSort(sort);
    prep.setThreads((uint16_t)std::max(1, threads));
    prep.setVerbose(verbose);
    prep.prepare(bamFiles, genomeFile);  // (refuses --use_csi without --build_csi)
    useCsi = useCsi || buildCsi;
    const double t1 = HostProfile::now();

    // ---- 2-junc (:329-348).  The run's contexts (up to ~100 GB of device memory) and page-locked rings are taken down on threads that
    // `juncDown` owns; whatever happens below, this function does not end -- by return or by exception -- before they have finished.
    banner("Identifying junctions and calculating metrics");
    const string juncDir = outputDir + "/2-junc", juncOut = juncDir + "/portcullis_all";
    const std::shared_ptr<JuncTeardown> juncDown = std::make_shared<JuncTeardown>();
    struct WaitAtExit {
        JuncTeardown& t;
        ~WaitAtExit() { t.wait(); }
    } waitAtExit{*juncDown};
    double waited = 0;
    {
        // deliberately never destroyed, as in junc: freeing every junction object one by one only takes time (filt reads the table back)
        JunctionBuilder& jb = *new JunctionBuilder(prepDir, juncOut);
        jb.setThreads((uint16_t)std::max(1, threads));
        jb.setStrandSpecific(strandedness);
        jb.setOrientation(orientation);
        jb.setExtra(extra);
        jb.setSeparate(separate);
        jb.setSource(source);
        jb.setUseCsi(useCsi);
        jb.setOutputExonGFF(exongff);
        jb.setOutputIntronGFF(introngff);
        jb.setVerbose(verbose);
        if (devices > 0) jb.setDevices(devices);
        if (deviceMem > 0) jb.setDeviceMem(deviceMem);
        jb.setTeardown(juncDown);
        jb.process();
    }
    const double t2 = HostProfile::now();

    // ---- 3-filt (:350-369).  The table is read back from the file: a junction parsed from it carries the printed six digits.  Loading
    // it, the rule files and the initial sets need no device and run beside junc's teardown; filter() calls back right before its first
    // device call, and only then is the teardown waited for.  Its own context lives inside filter().
    banner("Filtering junctions");
    const string filtOut = outputDir + "/3-filt/portcullis_filtered", juncTab = juncOut + ".junctions.tab";
    {
        JunctionFilter filter(prepDir, juncTab, filtOut);
        filter.setVerbose(verbose);
        filter.setSource(source);
        filter.setMaxLength(maxLength);
        filter.setCanonical(canonical);
        filter.setMinCov(minCov);
        filter.setTrain(true);
        filter.setSelfTrainDir(selfTrainDir);
        filter.setTrainingRule(trainingRule);
        filter.setThreads((uint16_t)std::max(1, threads));
        filter.setENN(false);
        filter.setOutputExonGFF(exongff);
        filter.setOutputIntronGFF(introngff);
        filter.setSaveBad(saveBad);
        filter.setSaveLayers(saveLayers);
        filter.setSaveFeatures(saveFeatures);
        filter.setSaveModels(saveModels);
        filter.setReferenceFile(referenceFile);
        filter.setBeforeDevice([&] { waited += juncDown->wait(); });
        filter.filter();
    }
    waited += juncDown->wait();  // (a route through filt that needed no device: the lenient rule file)
    const double t3 = HostProfile::now();

    // ---- bamfilt (:371-384)
    if (bamFilter) {
        banner("Filtering BAMs");
        BamFilter bf(filtOut + ".pass.junctions.tab", prep.getOutput().getSortedBamFilePath(), outputDir + "/portcullis.filtered.bam");
        bf.setUseCsi(useCsi);
        bf.setVerbose(verbose);
        bf.setThreads(threads);  // (as bamfilt -t: this program's BamFilter inflates, gathers and compresses on that many workers)
        bf.filter();
    }
    const double t4 = HostProfile::now();

    if (!keepTemp) {  // :386-391 -- the directory's links or copies, never what a link points at
        cout << "Cleaning temporary files...";
        cout.flush();
        prep.clean();
        cout << " done." << endl << endl;
    }
    printf("\nPortcullis completed.\nTotal runtime: %.1fs\n\n", HostProfile::now() - t0);
    if (prof)
        fprintf(stderr, "[host profile] full: prep %.3f s, junc %.3f s, filt %.3f s (of which %.3f s waiting for junc's teardown), bamfilt %.3f s, clean %.3f s\n", t1 - t0,
                t2 - t1, t3 - t2, waited, t4 - t3, HostProfile::now() - t4);
    return 0;
}

}  // namespace portcullis
