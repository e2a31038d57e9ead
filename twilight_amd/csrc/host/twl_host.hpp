// twilight_amd/csrc/host/twl_host.hpp -- host-side mirror of TWILIGHT's level-batch call surface.
//
// Same namespaces, type and function names, argument meaning and error behaviour as the reference
// (/root/reference/src/msa.hpp, phylogeny.hpp) for the DEFAULT_ALN path, so that the level kernel
// msa::progressive::gpu::alignmentKernel_GPU (align_gpu.cpp, calls the C ABI of include/twl_align.h)
// is injected exactly where the reference injects cpu::alignmentKernel_CPU (twilight-main.cpp:148).
// No Boost, no TBB: options are a plain struct, parallel loops are OpenMP.
#pragma once
#include "level_policy.hpp"

#include <cstdint>
#include <cstdlib>
#include <functional>
#include <map>
#include <stack>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <utility>
#include <vector>

namespace phylogeny {

using Profile = std::vector<std::vector<float>>;

// reference phylogeny.hpp:16-53
struct Node {
    Node(const std::string &id, float len);
    Node(const std::string &id, Node *par, float len);
    bool is_leaf() const { return identifier.compare(0, 4, "node") != 0; }
    void collectPostOrder(std::stack<Node *> &postStack);

    std::string identifier;
    Node *parent = nullptr;
    float branchLength = 0;
    size_t level = 1;
    std::vector<Node *> children;
    size_t numLeaves = 0;
    float weight = 0;
    bool placed = false;
    int grpID = -1;
    int schedIdx = -1;         // scratch of progressive::getProgressivePairs (position in its post-order walk)

    std::vector<int> seqsIncluded;
    Profile msaFreq;
    int cacheId = -1;          // device-resident mode: handle of the profile cached in the store (plays msaFreq; -1 = none)
    int alnLen = 0;
    int alnNum = 0;
    float alnWeight = 0;
    int getAlnNum(int) const { return alnNum; }
    int getAlnLen(int) const { return alnLen; }
};

// reference phylogeny.hpp:73-107 (the members the DEFAULT_ALN path touches)
struct Tree {
    size_t m_currInternalNode = 0;
    size_t m_maxDepth = 0;
    size_t m_numLeaves = 0;
    float m_meanDepth = 0;
    Node *root = nullptr;
    std::unordered_map<std::string, Node *> allNodes;   // iteration order is observable (reroot start leaf, tree.cpp:601-605)

    std::string newInternalNodeId() { return "node_" + std::to_string(++m_currInternalNode); }
    void calLeafNum();
    void calSeqWeight();
    void parseNewick(std::string &newick);
    void reroot(bool placement = false);      // placement: between placed nodes only (PLACE_W_TREE, after both reads)
    void convert2binaryTree();
    Tree *prune(std::unordered_set<std::string> &seqs);

    Tree() = default;
    explicit Tree(const std::string &newickFileName);
    struct FromText {};
    Tree(FromText, const std::string &newick);      // the first line of `newick`, as the constructor above takes the first line of its file
    Tree(Node *node, bool reroot);          // copy of the nodes that share node->grpID
    ~Tree();
};

void pruneTree(Tree *&T, std::unordered_set<std::string> &seqs);
void updateLevels(Node *node, size_t currentLevel);
// single-partition form of PartitionInfo::partitionTree (partitionInfo.cpp:75-85): every node joins group 0
void assignSinglePartition(Node *root);

// reference phylogeny.hpp:55-71 (partition.cpp): the tree cut into subtrees of at most maxPartitionSize leaves; grpID of every node = its subtree
struct PartitionInfo {
    size_t maxPartitionSize, minPartitionSize, numPartitions;
    std::unordered_map<std::string, std::pair<Node *, size_t>> partitionsRoot;      // root of every subtree by name, with its number of leaves
    PartitionInfo(size_t maxSize, size_t minSize, size_t num) : maxPartitionSize(maxSize), minPartitionSize(minSize), numPartitions(num) {}
    void partitionTree(Node *root);
    void bipartition(Node *root, Node *edge, Node *&tree1Root, Node *&tree2Root);
};
Tree *constructTreeFromPartitions(Node *root, PartitionInfo *P);      // phylogeny.cpp:13-39: the tree of the subtrees' roots
void updateSubrootInfo(Node *subroot, Tree *subT, int subtreeIdx);    // tree.cpp:519-526

}  // namespace phylogeny

char checkOnly(char c);
int letterIdx(char type, char c);

namespace msa {

enum Type { DEFAULT_ALN = 0, MERGE_MSA = 1, PLACE_WO_TREE = 2, PLACE_W_TREE = 3 };

using Node = phylogeny::Node;
using Tree = phylogeny::Tree;
using NodePair = std::pair<Node *, Node *>;
using NodePairVec = std::vector<NodePair>;
using stringPair = std::pair<std::string, std::string>;
using IntPair = std::pair<int, int>;
using IntPairVec = std::vector<IntPair>;
using FloatPair = std::pair<float, float>;
using alnPath = std::vector<int8_t>;
using Profile = std::vector<std::vector<float>>;

struct SequenceDB;

// reference msa.hpp:55-96; values are the CLI defaults of twilight-main.cpp:13-84
struct Option {
    int alnMode = DEFAULT_ALN;
    int gpuNum = 0;
    int cpuNum = 1;
    std::vector<int> gpuIdx;
    bool cpuOnly = false;
    int maxSubtree = INT32_MAX;
    float gappyVertical = 0.95f;
    float lenDev = 0;
    float maxAmbig = 0.1f;
    int maxLen = INT32_MAX;
    int minLen = 0;
    bool writeFiltered = false;
    bool debug = false;          // --check
    bool noFilter = true;        // !--filter
    bool reroot = true;          // !--rooted
    bool compressed = false;
    char type = 'n';
    bool alignGappy = true;
    std::string treeFile, seqFile, outFile;
    bool printDetail = false;    // -v
    // msa.hpp:179-180 (_CAL_PROFILE_TH, _UPDATE_SEQ_TH): 1000 in the reference; tests lower them per RUN (--test-cal-profile-th / --test-update-seq-th: small trees
    // then reach the cached-profile and compressed-group branches).  Per run since round 5: as process globals a handle with lowered thresholds changed every later one
    int calProfileTh = 1000, updateSeqTh = 1000;
    bool testForkHostStaged = false; // --test-fork-host-staged: the CLI forks one process per listed device for the host-staged kernel too (paths all-gathered through the library's communicator per level); lets the forked flow run on the CPU-check build
    bool testNoOwnership = false; // --test-no-ownership: a sharded run deals and exchanges every level (no subtree ownership below a cut)
    int testVirtualDevices = 0;  // --test-virtual-devices n: n replicas of the store on the first device (the several-replica path of the resident kernel on a one-GPU box)
    bool hostStaged = false;     // --host-staged: build profiles on the host and stage them per level (default: device-resident rows)
    std::string backboneAlnFile; // -a / --alignment: the existing alignment new sequences are placed into (alnMode PLACE_WO_TREE; with -t and --place-on-tree PLACE_W_TREE)
    bool placeOnTree = false;    // --place-on-tree: -a together with -t places the new sequences along the tree (place_tree.cpp)
    int testPlaceChunk = 0;      // --test-place-chunk n: placement aligns at most n sequences per level (default: sized to device memory)
    bool keepLength = false;     // --keep-length: placement (-a) leaves the backbone's columns as they are; the insertions of the new sequences are left out (place.cpp)
    std::string writeInsertionsFile; // --write-insertions: one "name<TAB>k<TAB>letters" line per run of letters --keep-length left out
    std::string msaDir;          // -f / --files: a directory of alignments to merge into one (alnMode MERGE_MSA)
    bool typeGiven = false;      // --type was given (a merge detects the type from its first file otherwise)
    bool buildTree = false;      // -i and -o without -t, -a or -f: the guide tree is built from the sequences (guide.cpp)
    std::string writeTreeFile;   // --write-tree: where the built tree is written
    int treeSeeds = 0;           // --tree-seeds S: the tree is built in two stages around S seed sequences (guide.cpp); 0: in one
    std::string treeText;        // the built tree as Newick text: read in place of treeFile (openTree)
    int iterations = 1;          // --iterations K: the run is repeated K times, runs 2 .. K on a tree computed from the alignment of the run before (retree.cpp)
    double maskGappy = 0.95;     // --mask-gappy T: a column with more than floor(T * N) gaps does not enter that tree's distances
    int retreeSeeds = 0;         // --retree-seeds S: those trees are built in two stages around S seed rows (retree.cpp); 0: in one
    bool adjustDirection = false;    // --adjust-direction: reverse-complemented records of -i are found from shared k-mers and turned before anything else reads them (strand.cpp)
    int directionSeeds = 0;          // --direction-seeds S: the directions are decided against S seed sequences; 0: the smallest S with S * S >= 4 N
    std::string writeDirectionsFile; // --write-directions: one "name<TAB>+|-" line per kept record, in input order
    std::unordered_set<std::string> reversedNames;      // the records of seqFile that adjustDirections found reversed: read reverse-complemented, written as _R_<name>
    int trimRule = -1;               // the rule by which the written rows lose columns (include/twl_trim.h): 0 --trim-gappy, 1 --trim-to; -1: they are written whole (trim.cpp)
    double trimGappy = 1.0;          // --trim-gappy T: a column with more than floor(T * N) gaps among the N written rows is left out
    std::string trimToName;          // --trim-to NAME: the columns in which the written row called NAME holds '-' are left out
    std::string writeColumnsFile;    // --write-columns: one "new<TAB>old<TAB>gaps" line per kept column
    bool allowCompare = false;       // set by the binary that carries the comparison (main.cpp) before it parses: --compare, --write-compare and --evaluate are options
    std::string compareFile;         // --compare REF: the written alignment is compared with this reference alignment (compare.cpp)
    std::string writeCompareFile;    // --write-compare: "#key<TAB>value" lines of the totals, then one line per written column
    std::string evaluateFile;        // --evaluate EST: no run, EST is compared with compareFile
    // set by the binary that carries the comparison (main.cpp): called by the writers of -o once the file is closed, with the records as they were written
    std::function<void(const std::vector<std::string> &, const std::vector<const char *> &, int)> compareWritten;
    bool allowScore = false;         // set by the binary that carries the score (main.cpp) before it parses: --score, --write-score and --score-alignment are options
    bool score = false;              // --score: the written alignment's affine sum-of-pairs score, one line on stderr (score.cpp)
    std::string writeScoreFile;      // --write-score: "#key<TAB>value" lines of the numbers, then name<TAB>letters<TAB>runs per written row
    std::string scoreAlignmentFile;  // --score-alignment FILE: no run, FILE is scored
    int scoreRun = 0;                // > 0: run k of --iterations, the prefix of the score line (retree.cpp)
    // set by the binary that carries the score (main.cpp): called by the writers of -o once the file is closed (behind compareWritten), and by --iterations
    // with the finished rows of every run but the last
    std::function<void(const std::vector<std::string> &, const std::vector<const char *> &, int)> scoreWritten;
    // set by the binary that carries the trim (main.cpp): trims the finished host rows of a run of runDefaultAlignment on an uploaded copy, returns the kept length
    std::function<int(SequenceDB *, Option *, int)> trimHostRows;
    // ... and on the run's own store (a twl_store *) in front of the last download; sets SequenceDB::trimmedLen, returns what to call once the rows are on the host
    std::function<std::function<void()>(SequenceDB *, Option *, void *)> trimResidentRows;
    // scoring flags (consumed by Params)
    float match = 18, mismatch = -8, transition = -4, gapOpen = -50, gapExtend = -5, xdrop = 600;
    bool hasGapEnds = false;
    float gapEnds = 0;
    bool wildcard = false;
    int blosum = 62;
    std::string matrixFile;      // -x / --matrix: user-defined substitution matrix (scoring-matrix.cpp:137-199)
};

// reference msa.hpp:98-109, ctor scoring-matrix.cpp:81-199
struct Params {
    float gapOpen, gapExtend, gapBoundary, xdrop, scaleFactor = 1;
    float **scoringMatrix;
    int matrixSize;
    Params(const Option &opt, char type);
    ~Params();
    Params(const Params &) = delete;
};

// reference msa.hpp:111-155
struct SequenceDB {
    struct SequenceInfo {
        int id;
        std::string name;
        std::string unalignedSeq;
        int len;
        bool lowQuality = false;
        int subtreeIdx;
        float weight;
        bool storage = false;
        bool borrowed = false;      // alnStorage points into SequenceDB::rowArena (device-resident mode hands all rows back in one block)
        int memLen = 0;
        char *alnStorage[2] = {nullptr, nullptr};
        static constexpr int timesBigger = 2;
        void changeStorage() { storage = !storage; }
        void memCheck(int len);
        SequenceInfo(int id_, const std::string &name_, std::string &seq, int subtreeIdx_, float weight_, bool debug);
        ~SequenceInfo();
    };
    int currentTask = 0;
    int finalAlnLen = 0;                           // the alignment length of the finished run (runDefaultAlignment sets it before its atEnd hook)
    int updateSeqTh = 1000;                        // Option::updateSeqTh of the run (updateAlignment has no Option)
    std::vector<SequenceInfo *> sequences;
    std::vector<Node *> fallback_nodes;
    std::unordered_map<std::string, SequenceInfo *> name_map;
    std::unordered_map<int, alnPath> subtreeAln;
    char *rowArena = nullptr;                      // owns the rows of sequences with `borrowed` set
    void *gpuCtx = nullptr;                        // per-run state of the GPU level kernels (progressive::gpu::RunCtx), freed through gpuCtxFree
    void (*gpuCtxFree)(void *) = nullptr;
    // set for a sharded run on the device-resident level kernel: aligns a prefix of the main pass's levels by subtree ownership (align_owned.cpp), returns how many
    std::function<size_t(Tree *, std::vector<std::vector<std::pair<Node *, Node *>>> &, Option *, Params &)> ownedPrefix;
    std::function<void(Tree *)> afterMainPass;    // set by the device-resident level kernel: bring rows/caches back to the host
    bool residentDeferred = false;                 // ... and that kernel runs the deferred pass on the resident rows too: they come back after it
    bool lazyRows = false;                         // library use (twl_msa.h): leave the rows in HBM after the main pass until somebody needs them
    bool trimRequested = false;                    // the run's output is trimmed (Option::trimRule): the download that is the run's last may trim the resident rows first
    bool lastDownload = false;                     // msaOnSubtree sets it in front of that download: no level rewrites rows behind it
    int trimmedLen = -1;                           // >= 0: that download trimmed the rows on the device; their length from there on
    void addSequence(int id, const std::string &name, std::string &seq, int subtreeIdx, float weight, bool debug);
    bool debug();      // --check: true when every aligned row reproduces its input sequence and all rows are equally long
    ~SequenceDB();
};

namespace io {
void readSequences(const std::string &fileName, SequenceDB *database, Option *option, Tree *&T);
void writeAlignment(const std::string &fileName, SequenceDB *database, int alnLen, const Option *option = nullptr);      // option: its reversedNames are written as _R_<name>
void writeFinalMSA(SequenceDB *database, Option *option, int alnLen);
char detectType(const std::string &seqFile);
// every record of a FASTA(.gz) file, in file order, as readSequences sees them: each(name, sequence)
// option: where fileName is its seqFile, the records named in its reversedNames arrive reverse-complemented
void readRecords(const std::string &fileName, const std::function<void(std::string &, std::string &)> &each, const Option *option = nullptr);
// every record of an alignment file (`kind`: "a backbone alignment", "an alignment"); returns the one length of its rows, -1 for a file without
// records; rows of two lengths end the run
int32_t readAlignedRows(const std::string &fileName, const char *kind, std::vector<std::string> &names, std::vector<std::string> &rows);
// plain FASTA of rows that all have W columns: record k is names[k] and the W bytes at rows[k]
// option: the records from firstRenamable on whose names are in its reversedNames are written as _R_<name>
void writeRecords(const std::string &fileName, const std::vector<const std::string *> &names, const std::vector<const char *> &rows, int W, const Option *option = nullptr,
                  size_t firstRenamable = 0);
}  // namespace io

using alnFunction = std::function<void(Tree *, NodePairVec &, SequenceDB *, Option *, Params &)>;

namespace alignment_helper {
void calculateProfile(float *profile, NodePair &nodes, SequenceDB *database, Option *option, int32_t memLen);
void removeGappyColumns(float *hostFreq, NodePair &nodes, Option *option, std::pair<IntPairVec, IntPairVec> &gappyColumns, int32_t memLen,
                        IntPair &lens, int currentTask);
void calculatePSGP(float *hostFreq, float *hostGapOp, float *hostGapEx, NodePair &nodes, SequenceDB *database, Option *option, int memLen,
                   IntPair offset, IntPair lens, Params &param);
void getConsensus(Option *option, float *profile, std::string &consensus, int len);
void pairwiseGlobal(const std::string &seq1, const std::string &seq2, alnPath &path, Params &param);
void addGappyColumnsBack(alnPath &aln_before, alnPath &aln_after, std::pair<IntPairVec, IntPairVec> &gappyColumns, Params &param,
                         IntPair rgcLens, stringPair orgSeqs);
void updateAlignment(NodePair &nodes, SequenceDB *database, Option *option, alnPath &aln);
void updateFrequency(NodePair &nodes, SequenceDB *database, alnPath &aln, FloatPair weights);
void fallback2cpu(std::vector<int> &fallbackPairs, NodePairVec &nodes, SequenceDB *database, Option *option);
}  // namespace alignment_helper

namespace progressive {
void getProgressivePairs(std::vector<std::pair<NodePair, int>> &alnOrder, std::stack<Node *> postStack, int grpID, int mode);
void scheduling(Node *root, std::vector<NodePairVec> &levels, int mode);
void updateNode(Tree *tree, NodePairVec &nodes, SequenceDB *database);
void progressiveAlignment(Tree *T, SequenceDB *database, Option *option, std::vector<NodePairVec> &levels, Params &param, alnFunction kernel);
// Subtree ownership of a sharded run: levels [0, cut] are aligned by the owner of each pair's subtree alone (owner[level][pair]), the rest dealt per level.
struct OwnershipPlan { int cut = -1; int subtrees = 0; std::vector<std::vector<int>> owner; std::vector<long long> load; };
OwnershipPlan planOwnership(Tree *T, const std::vector<NodePairVec> &levels, int world);
// `deferredKernel` aligns the deferred sequences against the root in the second pass; the reference hard-wires
// cpu::alignmentKernel_CPU there (progressive.cpp:291).
void msaOnSubtree(Tree *T, SequenceDB *database, Option *option, Params &param, alnFunction kernel, alnFunction deferredKernel);
void updateAlignment(Node *node, SequenceDB *database);

// What one pair needs before / after the DP (alignment-cpu.cpp:50-93 and :136-175), shared by every level kernel.
// A float buffer that is either owned (per-pair vector) or a slot of the level's flat staging arrays (align_gpu.cpp).
struct FloatBuf {
    std::vector<float> own;
    float *ext = nullptr;
    float *data() { return ext ? ext : own.data(); }
    const float *data() const { return ext ? ext : own.data(); }
    void assign(size_t n, float v) { ext = nullptr; own.assign(n, v); }
    void bind(float *slot, size_t n) { ext = slot; std::fill(slot, slot + n, 0.0f); }
};
struct PairInputs : PairShape {                      // (level_policy.hpp: lengths, sequence counts, low-quality flags)
    FloatBuf freq, gapOp, gapEx;                     // freq[2][memLen][P], gapOp/gapEx[2][memLen]
    std::pair<IntPairVec, IntPairVec> gappyColumns;
    stringPair consensus;
    int32_t memLen;
};
// the lowQuality flag of a side's first sequence, for lowQualitySide (a side of several sequences may start with a compressed group: no flag)
inline bool firstSeqLowQuality(const Node *node, const SequenceDB *database)
{
    const int s = node->seqsIncluded.empty() ? -1 : node->seqsIncluded[0];
    return s >= 0 && s < (int)database->sequences.size() && database->sequences[s]->lowQuality;
}
// With slots given, the pair's buffers are built in place there with row stride `stride` (>= max(refLen, qryLen)); the stride
// is only an address stride (alignment-cpu.cpp:13-30 uses max(refLen, qryLen)), it does not enter any value.
void preparePair(NodePair &nodes, SequenceDB *database, Option *option, Params &param, PairInputs &in, float *freqSlot = nullptr,
                 float *gapOpSlot = nullptr, float *gapExSlot = nullptr, int stride = 0);
// Returns false when the pair must be deferred (fallbackPairs), true when it was written back.
bool finishPair(NodePair &nodes, SequenceDB *database, Option *option, Params &param, PairInputs &in, alnPath &aln_wo_gc);

namespace gpu {
void alignmentKernel_GPU(Tree *T, NodePairVec &alnPairs, SequenceDB *database, Option *option, Params &param);
void beginInit(Option *option);   // optional: start device initialisation early, on a helper thread
// Device-resident variant (include/twl_level.h): rows and cached profiles stay in HBM during the main progressive pass; profile
// building, gappy-column removal, gap penalties and the row write-back run as kernels.  The deferred pass (currentTask 1) runs on
// the resident rows too; currentTask 2, or a run whose rows are back on the host, falls through to alignmentKernel_GPU.
void alignmentKernel_Resident(Tree *T, NodePairVec &alnPairs, SequenceDB *database, Option *option, Params &param);
struct LevelTotals { uint64_t band_cells = 0, pairs = 0, relaunched = 0, nominal_cells = 0 /* sum of R*Q over the pairs this process's level calls saw (all of them on one GPU) */; double kernel_ms = 0, total_ms = 0, prepare_ms = 0, stage_ms = 0, call_ms = 0, finish_ms = 0, dev_prepare_ms = 0, dev_commit_ms = 0, exchange_ms = 0; };
// One level-kernel call, as the reference's per-level report line (progressive.cpp:178-189) plus what the DP did in it.
struct LevelRecord { int32_t pairs = 0, task = 0; uint64_t band_cells = 0, relaunched = 0; double kernel_ms = 0, level_ms = 0, exchange_ms = 0; int32_t matrix_mode = -1, speculative = 0;
                     int32_t mt_predicted = 0, mt_inline = 0; char kernel[160] = {0}; };
// Several processes (one per GPU) aligning ONE family together: every process runs the same host flow on its own replica, aligns
// the pairs dealt to its rank and receives the other ranks' paths through `exchange` (an all-gather of equal-sized host blocks:
// send = this rank's block, recv = [world][bytes_per_rank]; returns 0 on success).  twilight_amd/dist.py provides it over
// torch.distributed (backend nccl = RCCL over xGMI on GPUs, gloo in the CPU tests).
using ExchangeFn = int (*)(void *user, const void *send, int64_t bytes_per_rank, void *recv);
// exchangeDev: the same all-gather on DEVICE buffers (this process's GPU); with it the device-resident level kernel keeps the paths in
// HBM end to end (align -> gappy columns back -> pack -> all-gather -> unpack -> write-back)
struct Shard { int rank = 0, world = 1; ExchangeFn exchange = nullptr; void *user = nullptr; ExchangeFn exchangeDev = nullptr; void *userDev = nullptr;
               bool rccl = false; };      // rccl: the all-gathers are the library's own (twl_comm_all_gather*, RCCL from C++), no callback
// Communicator of a sharded run on this process's device (twl_comm_init); the two all-gathers the level kernels use when Shard::rccl is set.
int initRcclShard(SequenceDB *database, Option *option, int rank, int world, const void *id128);      // 0, or the code of twl_comm_init
void ensureDevicesUp(Option *option);      // joins the twl_init started by beginInit
// Subtree ownership of a sharded run (align_owned.cpp): levels [0, returned) of the main pass are done when it returns.
size_t ownedPrefix(Tree *T, std::vector<NodePairVec> &levels, SequenceDB *database, Option *option, Params &param);
// Per-run state of the level kernels; hangs off SequenceDB::gpuCtx so that several runs can live in one process.
struct RunCtx;
RunCtx &ctxOf(SequenceDB *database);
void setShard(SequenceDB *database, const Shard &shard);
const std::vector<LevelRecord> &levelRecords(SequenceDB *database);
const LevelTotals &runTotals(SequenceDB *database);
// Device-resident mode: create the store (sequences into HBM) ahead of the first level, e.g. before a timed region.
void uploadSequences(SequenceDB *database, Option *option);
// Rows (and the root's cached profile) back to the host, if they are still in HBM.
void downloadRows(SequenceDB *database, Tree *T);
}

}  // namespace progressive

// DEFAULT_ALN driver shared by the product CLI and the oracle's end-to-end checker (twilight-main.cpp:121-176,
// single partition): tree -> partition -> reroot -> read sequences -> msaOnSubtree -> write MSA.  Returns the MSA length.
// atEnd (optional) sees the run's SequenceDB after the output was written and before it is destroyed (the CLI reads the run's totals there)
int runDefaultAlignment(Option &option, alnFunction kernel, alnFunction deferredKernel, bool writeOutput = true,
                        const std::function<void(SequenceDB *)> &atEnd = nullptr, const std::function<void(SequenceDB *)> &beforeAlign = nullptr);
// allowPlacement: the binary carries the placement mode (twilight-mi355x): -a/--alignment with -i/-o and no -t selects PLACE_WO_TREE
//                 ... and -a with -t, -i, -o and --place-on-tree selects PLACE_W_TREE (without the flag -a with -t is refused)
// allowMerge: the binary carries the merge mode as well: -f/--files with -o and none of -t, -i, -a selects MERGE_MSA
// allowSubtrees: the binary carries the subtree mode too: -m/--max-subtree N with -t, -i, -o sets Option::maxSubtree
// allowGuide: the binary builds the guide tree itself when none is given: -i and -o without -t, -a or -f sets Option::buildTree
//             ... and knows --iterations K, --mask-gappy T and --retree-seeds S (retree.cpp); without it all three are unsupported options
// allowTrim: the binary can write its alignment without the gappy columns: --trim-gappy T, --trim-to NAME and --write-columns FILE (trim.cpp);
//            without it all three are unsupported options
bool parseCommandLine(int argc, char **argv, Option &option, bool allowPlacement = false, bool allowMerge = false, bool allowSubtrees = false, bool allowGuide = false,
                      bool allowTrim = false);
// Option::allowCompare, set before the call: the binary can compare what it writes with a reference alignment: --compare REF, --write-compare FILE,
// --evaluate EST (compare.cpp); without it all three are unsupported options
// --compare (compare.cpp, libtwl_host.so): gives a run with Option::compareFile its hook behind the writers (seqdb_io.cpp); the rows as they were
// written are matched with the reference's rows by name and compared on the device (include/twl_compare.h).
void enableCompare(Option &option);
// --evaluate EST --compare REF: no run, the two files compared.  Returns the process's exit code.
int runEvaluate(Option &option);
// Option::allowScore, set before the call: the binary can score what it writes: --score, --write-score FILE, --score-alignment FILE (score.cpp);
// without it all three are unsupported options.
// --score (score.cpp, libtwl_host.so): gives a run with Option::score its hook behind the writers (seqdb_io.cpp); the rows as they were written go
// into a store and twl_store_score_rows (include/twl_score.h) counts the integers the score is computed from.
void enableScore(Option &option);
// --score-alignment FILE: no run, the file scored.  Returns the process's exit code.
int runScoreAlignment(Option &option);
// --trim-gappy / --trim-to (trim.cpp, libtwl_host.so): gives a run with Option::trimRule its two trim hooks; every mode then writes its rows without
// the columns the rule leaves out, decided and compacted on the device (include/twl_trim.h).
void enableTrim(Option &option);
// The guide tree of a run: from option.treeText when the run built it, from the file option.treeFile otherwise; the same parser either way.
Tree *openTree(const Option &option);
// No -t (guide.cpp, libtwl_host.so): the sequences of option.seqFile -> shared k-mer counts of all pairs on the device -> distances -> UPGMA ->
// Newick text, written to option.writeTreeFile when that is set.  Returns the text.
// With option.treeSeeds > 0 the tree is built in two stages (section 4g): seeds, clusters around them, a tree per cluster grafted onto the seeds' tree.
std::string buildGuideTree(Option &option);
// --adjust-direction (strand.cpp, libtwl_host.so): the strand of every record of option.seqFile, decided on the device from the
// k-mers it shares with seed sequences and with their reverse complements (include/twl_strand.h).  Fills option.reversedNames and writes
// option.writeDirectionsFile; runs before anything else opens the input.  With -a the seeds are backbone rows, which are never turned.
void adjustDirections(Option &option);
// What buildGuideTree refuses about a sequence name (it could not be a leaf of a written tree): ends the run with a message.
void refuseName(const std::string &name);
// --iterations K, K >= 2 (retree.cpp, libtwl_host.so): the default alignment K times; after every run but the last the guide tree is computed anew
// from the finished rows (pair counts on the device, include/twl_retree.h; distances, UPGMA and text on the host).  The first tree is the
// user's (-t) or the k-mer tree.  Only the last alignment is written; option.writeTreeFile receives the tree it was built on.  Returns its length.
// With option.retreeSeeds > 0 the trees are rebuilt in two stages (section 4j; include/twl_retree_set.h), for up to 2^20 sequences.
int runIterations(Option &option);
// PLACE_WO_TREE (place.cpp, libtwl_host.so): the sequences of option.seqFile placed into the alignment option.backboneAlnFile, written to
// option.outFile.  Returns the final alignment length.
int runPlacement(Option &option);
// PLACE_W_TREE (place_tree.cpp, libtwl_host.so): the sequences of option.seqFile placed into the alignment option.backboneAlnFile where the tree
// option.treeFile says they belong, written to option.outFile.  Returns the final alignment length.
int runPlacementOnTree(Option &option);
// The host half of that mode up to the level schedule (place_tree.cpp; tests/place_tree_dump.cpp prints it): both reads, the reroot between placed
// nodes, the placed marks and the backbone group of every placed node.  subT: the whole tree's copy; returns the tree of the placed nodes
// (getPlacementTree, sequencedb.cpp:148-246, without its host loop over the all-gap columns: the groups still have the backbone's width).
struct PlacementGroups { std::vector<Node *> nodes; int32_t backboneLen = 0, backboneRows = 0; };      // nodes: the placement tree's inner nodes that bring members, by name
Tree *readPlacementInputs(Option &option, SequenceDB &database, Tree *subT, PlacementGroups &groups);
// MERGE_MSA (merge.cpp, libtwl_host.so): the alignments found under option.msaDir merged into one, written to option.outFile.  Returns the
// final alignment length.
int runMerge(Option &option);
// DEFAULT_ALN with -m N (subtrees.cpp, libtwl_host.so): the guide tree cut into subtrees of at most option.maxSubtree leaves, every subtree
// aligned on its own, their profiles merged along the tree of subtrees, written to option.outFile.  Returns the final alignment length,
// or -1 when the tree is not split (at most N leaves): nothing has been done then and the caller takes the default path.
int runSubtrees(Option &option);

}  // namespace msa
