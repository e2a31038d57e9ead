// twilight_amd/csrc/host/main.cpp -- `twilight-mi355x`: TWILIGHT's tree+sequences mode with the MI355X level kernel.
//   twilight-mi355x -t tree.nwk -i seqs.fa -o out.aln [-v] [--check] [--gpu-index 0,1,...] [scoring flags as in TWILIGHT]
//   twilight-mi355x -a backbone.aln -i new.fa -o out.aln [...]   (built with TWL_PLACE: placement without a tree, place.cpp)
//   twilight-mi355x -a backbone.aln -i new.fa -o out.aln --keep-length [--write-insertions FILE] [...]   (TWL_PLACE: the backbone's columns kept, insertions left out, place.cpp)
//   twilight-mi355x -t tree.nwk -a backbone.aln -i new.fa -o out.aln --place-on-tree [...] (TWL_PLACE: placement along the tree, place_tree.cpp)
//   twilight-mi355x -f DIR -o out.aln [...]                      (built with TWL_MERGE: the alignments of a directory merged, merge.cpp)
//   twilight-mi355x -t tree.nwk -i seqs.fa -o out.aln -m N [...] (built with TWL_SUBTREE: the tree aligned in subtrees of at most N leaves, subtrees.cpp)
//   twilight-mi355x -i seqs.fa -o out.aln [--write-tree t.nwk] [--tree-seeds S]   (built with TWL_GUIDE: no tree given, the guide tree is built from the sequences, guide.cpp)
//   twilight-mi355x [-t tree.nwk | -a backbone.aln] -i seqs.fa -o out.aln --adjust-direction [--direction-seeds S] [--write-directions FILE]   (TWL_GUIDE: reverse-complemented records turned first, strand.cpp)
//   twilight-mi355x <any form that writes -o> --compare ref.aln [--write-compare FILE]; twilight-mi355x --evaluate est.aln --compare ref.aln   (TWL_COMPARE: compare.cpp)
//   twilight-mi355x <any form that writes -o> --score [--write-score FILE]; twilight-mi355x --score-alignment est.aln   (TWL_SCORE: score.cpp)
//   twilight-mi355x [-t tree.nwk] -i seqs.fa -o out.aln --iterations K [--mask-gappy T] [--retree-seeds S]   (TWL_GUIDE: the run K times, the tree rebuilt from every alignment but the last, retree.cpp)
#include "twl_host.hpp"

#include "../../../include/twl_align.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstring>
#include <iostream>
#include <new>
#include <thread>
#include <vector>

#include <csignal>
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/prctl.h>
#include <sys/wait.h>
#include <unistd.h>

#ifndef TWL_BUILD_STAMP
#define TWL_BUILD_STAMP "unstamped"
#endif
// digest of this artefact's sources, headers and flags (__graft_entry__.build() rebuilds when the file does not carry the current one)
__attribute__((used)) static const char twl_build_stamp[] = "TWLSTAMP:" TWL_BUILD_STAMP ";";

// --gpu-index a,b,...: one PROCESS per GPU, forked here before anything touches the GPU.  The ranks align the same family
// together: the pairs of every level are dealt to them, each aligns its share on its device, and the final paths meet in ONE ncclAllGather
// per level, HBM to HBM over xGMI, made by the library itself (include/twl_align.h, twl_comm_*).  The 128-byte communicator id goes from
// rank 0 to the others through a page the processes share; rank 0 (this process) writes the MSA.
//
// A rank that fails must not leave the others behind: they may be spinning on the page or blocked inside ncclCommInitRank / an
// all-gather, which no return code ever leaves.  So: every rank marks the page `failed` from an exit hook unless it got to its normal end; the
// children ask the kernel for SIGTERM when their parent dies and watch the page and getppid() from a thread of their own; rank 0 reaps its children
// from a watchdog thread while the run is going on -- a child that ends badly, or a page marked failed, ends the whole run at once: the children
// are killed and the process leaves with an error.  Nothing is ever re-executed.
namespace {
struct SharedPage { std::atomic<int> ready; std::atomic<int> failed; char id[TWL_COMM_ID_BYTES]; };
SharedPage *g_page = nullptr;
std::atomic<int> g_finishedOk{0};
void markFailedAtExit() { if (g_page && !g_finishedOk.load()) g_page->failed = 1; }
void killAll(const std::vector<pid_t> &kids) { for (pid_t k : kids) if (k > 0) kill(k, SIGTERM); }
}

int main(int argc, char **argv)
{
    msa::Option option;
#ifdef TWL_PLACE
    const bool placement = true;
#else
    const bool placement = false;
#endif
#ifdef TWL_MERGE
    const bool merging = true;
#else
    const bool merging = false;
#endif
#ifdef TWL_SUBTREE
    const bool subtrees = true;
#else
    const bool subtrees = false;
#endif
#ifdef TWL_GUIDE
    const bool guide = true;
#else
    const bool guide = false;
#endif
#ifdef TWL_TRIM
    const bool trim = true;
#else
    const bool trim = false;
#endif
#ifdef TWL_COMPARE
    const bool compare = true;
#else
    const bool compare = false;
#endif
    option.allowCompare = compare;
#ifdef TWL_SCORE
    const bool score = true;
#else
    const bool score = false;
#endif
    option.allowScore = score;
    if (!msa::parseCommandLine(argc, argv, option, placement, merging, subtrees, guide, trim)) {
        std::cerr << "usage: twilight-mi355x -t <tree.nwk> -i <sequences.fa[.gz]> -o <out.aln> [-r 0.95] [--type n|p] [--match 18 --mismatch -8 --transition -4\n"
                     "        --gap-open -50 --gap-extend -5 --gap-ends X --xdrop 600] [-w] [--rooted] [--filter] [--check] [-v] [--gpu-index 0,1] [--host-staged]\n";
        if (placement) std::cerr << "       twilight-mi355x -a <backbone.aln[.gz]> -i <new_sequences.fa[.gz]> -o <out.aln> [scoring and filtering flags as above] [--gpu-index 0]\n";
        if (placement) std::cerr << "       twilight-mi355x -a <backbone.aln[.gz]> -i <new_sequences.fa[.gz]> -o <out.aln> --keep-length [--write-insertions <file>] [flags of the form above]\n"
                                    "        (the backbone's columns stay as they are: its rows are written byte for byte, every new sequence at the backbone's length; the letters a new sequence\n"
                                    "         has between two backbone columns are left out, and --write-insertions lists them as name<TAB>backbone columns in front<TAB>letters; no -f, --place-on-tree)\n";
        if (placement) std::cerr << "       twilight-mi355x -t <tree.nwk> -a <backbone.aln[.gz]> -i <new_sequences.fa[.gz]> -o <out.aln> --place-on-tree [flags of the first form; one GPU, no --host-staged, no -m]\n"
                                    "        (the tree holds the backbone's rows and the new sequences; the backbone falls into groups along the tree, which are re-aligned against each other)\n";
        if (merging) std::cerr << "       twilight-mi355x -f <directory of alignments (.gz too), searched recursively> -o <out.aln> [scoring flags as above] [-r 0.95] [--type n|p] [-v] [--gpu-index 0]\n"
                                  "        (every file must hold rows of one length; the output lists the files in sorted order, rows in file order, gaps as '-')\n";
        if (subtrees) std::cerr << "       twilight-mi355x -t <tree.nwk> -i <sequences.fa[.gz]> -o <out.aln> -m <max. leaves per subtree> [flags of the first form; one GPU, no --host-staged]\n"
                                   "        (the tree is cut into subtrees that are aligned one after the other, their profiles are merged along the tree of subtrees;\n"
                                   "         the output lists the subtrees in ascending index, rows in input order)\n";
        if (guide) std::cerr << "       twilight-mi355x -i <sequences.fa[.gz]> -o <out.aln> [--write-tree <tree.nwk>] [--tree-seeds S] [-m N] [flags of the first form; one GPU, no --host-staged]\n"
                                "        (no -t: the guide tree is built from the k-mers the sequences share, at most 16384 sequences, and the run goes on as with -t on that tree;\n"
                                "         --tree-seeds S builds it in two stages around S seed sequences, for more sequences than that: S near twice the square root of their number)\n"
                                "       twilight-mi355x [-t <tree.nwk>] -i <sequences.fa[.gz]> -o <out.aln> --iterations K [--mask-gappy 0.95] [--retree-seeds S] [--write-tree <tree.nwk>] [scoring flags; one GPU]\n"
                                "        (K = 1 .. 5 runs: after every run but the last the guide tree is computed anew from the alignment, over the columns in which at most\n"
                                "         the part --mask-gappy of the rows holds a gap; at most 16384 sequences; no -a, -f, -m, --filter, --host-staged; only the last alignment is written;\n"
                                "         --retree-seeds S computes those trees in two stages around S seed rows, for more sequences than that: S near twice the square root of their number)\n";
        if (guide) std::cerr << "       twilight-mi355x [-t <tree.nwk> | -a <backbone.aln>] -i <sequences.fa[.gz]> -o <out.aln> --adjust-direction [--direction-seeds S] [--write-directions <file>] [flags of that form; one GPU]\n"
                                "        (nucleotides: records that lie reverse-complemented are found from the 6-mers they share with S seed sequences and with the seeds' reverse complements,\n"
                                "         turned before anything else reads them and written as _R_<name>; S defaults to the smallest S with S * S >= 4 N; with -a the seeds are backbone rows and only\n"
                                "         new sequences are turned; no -f, --place-on-tree, --host-staged; --write-directions lists name<TAB>+ or - per kept record, in input order)\n";
        if (trim) std::cerr << "       every form above but --keep-length: [--trim-gappy T | --trim-to NAME] [--write-columns <file>]   (one GPU, no --host-staged)\n"
                               "        (the alignment is written without its gappy columns: --trim-gappy keeps the columns in which at most floor(T * N) of the N written rows hold '-',\n"
                               "         T in [0, 1]; --trim-to keeps the columns in which the written row called NAME holds a letter; --write-columns lists new<TAB>old<TAB>gaps per kept column)\n";
        if (compare) std::cerr << "       every form above but --adjust-direction, --keep-length, --trim-gappy, --trim-to: --compare <reference.aln[.gz]> [--write-compare <file>]   (one GPU, no --host-staged)\n"
                                  "        (the written rows are matched by name with the rows of the reference alignment and compared with them on the device; one line on stderr:\n"
                                  "         shared residue pairs over the reference's pairs (SP), over the output's pairs (modeler), reference columns recovered whole (TC);\n"
                                  "         --write-compare lists #key<TAB>value per number of that line, then column<TAB>letters<TAB>pairs<TAB>shared<TAB>distinct<TAB>recovered per written column)\n"
                                  "       twilight-mi355x --evaluate <alignment.aln[.gz]> --compare <reference.aln[.gz]> [--write-compare <file>] [--gpu-index 0] [-v]   (no run: the two files are compared)\n";
        if (score) std::cerr << "       every form above but --keep-length, --trim-gappy, --trim-to: --score [--write-score <file>]   (one GPU, no --host-staged)\n"
                                "        (the affine sum-of-pairs score of the written rows under the run's own substitution scores and gap penalties, counted on the device in exact integers; one line on stderr:\n"
                                "         score: rows N columns W pairs P letters L gapcols G runs R terminal RT/GT score S per_pair S/P; a pair with a letter outside the alphabet scores 0, with -w too;\n"
                                "         with --iterations one line per run, prefixed run k; --write-score lists #key<TAB>value per number and per sub[a][b], then name<TAB>letters<TAB>runs per written row)\n"
                                "       twilight-mi355x --score-alignment <alignment.aln[.gz]> [--type n|p] [scoring flags] [--write-score <file>] [--gpu-index 0] [-v]   (no run: the file is scored)\n";
        return 1;
    }
#ifdef TWL_SCORE
    if (!option.scoreAlignmentFile.empty()) return msa::runScoreAlignment(option);
    msa::enableScore(option);
#endif
#ifdef TWL_COMPARE
    if (!option.evaluateFile.empty()) return msa::runEvaluate(option);
    msa::enableCompare(option);
#endif
#ifdef TWL_TRIM
    msa::enableTrim(option);
#endif
#ifdef TWL_GUIDE
    if (option.adjustDirection) msa::adjustDirections(option);      // one process, one GPU (parseCommandLine refused more); every later read of -i sees the oriented records
    if (option.iterations > 1) {                     // one process, one GPU (parseCommandLine refused more); builds the first tree itself where none is given
        const auto ti = std::chrono::high_resolution_clock::now();
        const int W = msa::runIterations(option);
        std::cerr << "Wrote " << option.outFile << " (length " << W << ") in " << std::chrono::duration<double>(std::chrono::high_resolution_clock::now() - ti).count() << " s\n";
        return 0;
    }
    if (option.buildTree) option.treeText = msa::buildGuideTree(option);      // one process, one GPU (parseCommandLine refused more); from here on the run is the run of -t on this text
#endif
#ifdef TWL_MERGE
    if (option.alnMode == msa::MERGE_MSA) {          // one process, one GPU (parseCommandLine refused more)
        const auto tm = std::chrono::high_resolution_clock::now();
        const int W = msa::runMerge(option);
        std::cerr << "Wrote " << option.outFile << " (length " << W << ") in " << std::chrono::duration<double>(std::chrono::high_resolution_clock::now() - tm).count() << " s\n";
        return 0;
    }
#endif
#ifdef TWL_PLACE
    if (option.alnMode == msa::PLACE_W_TREE) {       // one process, one GPU (parseCommandLine refused more)
        const auto tp = std::chrono::high_resolution_clock::now();
        const int W = msa::runPlacementOnTree(option);
        std::cerr << "Wrote " << option.outFile << " (length " << W << ") in " << std::chrono::duration<double>(std::chrono::high_resolution_clock::now() - tp).count() << " s\n";
        return 0;
    }
    if (option.alnMode == msa::PLACE_WO_TREE) {      // one process, one GPU (parseCommandLine refused more)
        const auto tp = std::chrono::high_resolution_clock::now();
        const int W = msa::runPlacement(option);
        std::cerr << "Wrote " << option.outFile << " (length " << W << ") in " << std::chrono::duration<double>(std::chrono::high_resolution_clock::now() - tp).count() << " s\n";
        return 0;
    }
#endif
#ifdef TWL_SUBTREE
    if (option.maxSubtree != INT32_MAX) {            // one process, one GPU (parseCommandLine refused more); -1: the tree is not split, the run is the default run
        const auto ts = std::chrono::high_resolution_clock::now();
        const int W = msa::runSubtrees(option);
        if (W >= 0) {
            std::cerr << "Wrote " << option.outFile << " (length " << W << ") in " << std::chrono::duration<double>(std::chrono::high_resolution_clock::now() - ts).count() << " s\n";
            return 0;
        }
    }
#endif
    auto t0 = std::chrono::high_resolution_clock::now();
    int rank = 0;
    const std::vector<int> allDevices = option.gpuIdx;
    const int world = (allDevices.size() > 1 && (!option.hostStaged || option.testForkHostStaged) && option.testVirtualDevices == 0) ? (int)allDevices.size() : 1;
    SharedPage *page = nullptr;
    std::vector<pid_t> kids;
    if (world > 1) {
        void *mem = mmap(nullptr, sizeof(SharedPage), PROT_READ | PROT_WRITE, MAP_SHARED | MAP_ANONYMOUS, -1, 0);
        if (mem == MAP_FAILED) { std::cerr << "ERROR: mmap of the page the ranks share failed.\n"; return 1; }
        page = new (mem) SharedPage();
        page->ready = 0; page->failed = 0;
        const pid_t parent = getpid();
        for (int r = 1; r < world; ++r) {
            const pid_t pid = fork();
            if (pid < 0) { std::cerr << "ERROR: fork failed.\n"; page->failed = 1; killAll(kids); for (pid_t k : kids) waitpid(k, nullptr, 0); return 1; }
            if (pid == 0) {
                rank = r; kids.clear();
                prctl(PR_SET_PDEATHSIG, SIGTERM);
                if (getppid() != parent) _exit(1);      // (the parent was gone before the request took effect)
                break;
            }
            kids.push_back(pid);
        }
        g_page = page;
        atexit(markFailedAtExit);
        if (rank != 0) {
            // a child blocked in a collective never sees a return code: this thread ends the process when the run has failed elsewhere
            std::thread([page, parent]() {
                for (;;) {
                    if (page->failed.load() || getppid() != parent) _exit(1);
                    std::this_thread::sleep_for(std::chrono::milliseconds(20));
                }
            }).detach();
        }
        option.gpuIdx.assign(1, allDevices[rank]);
        if (rank != 0) {       // the other ranks say nothing unless asked to (TWL_DEBUG)
            option.printDetail = false;
            if (!getenv("TWL_DEBUG")) { const int nul = open("/dev/null", O_WRONLY); if (nul >= 0) { dup2(nul, 1); dup2(nul, 2); close(nul); } }
        }
    }
    // rank 0: reap the children while the run is going on
    std::thread watchdog;
    if (world > 1 && rank == 0) {
        watchdog = std::thread([&]() {
            std::vector<pid_t> left = kids;
            while (!left.empty()) {
                bool bad = page->failed.load() != 0;
                for (pid_t &k : left) {
                    int st = 0;
                    const pid_t r = waitpid(k, &st, WNOHANG);
                    if (r == 0) continue;
                    if (r < 0 || !WIFEXITED(st) || WEXITSTATUS(st) != 0) bad = true;
                    k = 0;
                }
                left.erase(std::remove(left.begin(), left.end(), (pid_t)0), left.end());
                if (bad) {
                    std::cerr << "ERROR: a rank failed; ending the run.\n";
                    page->failed = 1;
                    killAll(left);
                    for (pid_t k : left) waitpid(k, nullptr, 0);
                    _exit(1);      // (this process may be inside a collective that will never return)
                }
                if (!left.empty()) std::this_thread::sleep_for(std::chrono::milliseconds(20));
            }
        });
    }
    if (!option.buildTree && !option.adjustDirection) msa::progressive::gpu::beginInit(&option);      // (a run that built its tree or decided directions has its device up already)
    // exit handlers run last-registered first: registered again behind whatever the GPU runtime registered while it came up, the mark is set
    // BEFORE the runtime's own teardown, which may block while other ranks sit in a collective
    if (world > 1) atexit(markFailedAtExit);
    // both passes run on the GPU level kernel (the reference hard-wires its CPU kernel for the deferred pass)
    msa::alnFunction kernel = msa::progressive::gpu::alignmentKernel_Resident;
    if (option.hostStaged) kernel = msa::progressive::gpu::alignmentKernel_GPU;
    msa::progressive::gpu::LevelTotals g;      // the run's totals (they live with the run's SequenceDB)
    auto beforeAlign = [&](msa::SequenceDB *db) {
        if (world == 1) return;
        if (rank == 0) {
            msa::progressive::gpu::ensureDevicesUp(&option);
            if (twl_comm_unique_id(page->id) != TWL_OK) { std::cerr << "ERROR: " << twl_last_error() << '\n'; page->failed = 1; exit(1); }
            atexit(markFailedAtExit);      // (the devices are up: behind the runtime's handlers)
            page->ready = 1;
        } else {
            while (!page->ready.load() && !page->failed.load()) std::this_thread::sleep_for(std::chrono::milliseconds(1));      // (the watcher thread covers a parent that is gone)
            if (page->failed.load()) exit(1);
        }
        const int rcComm = msa::progressive::gpu::initRcclShard(db, &option, rank, world, page->id);
        if (rcComm != TWL_OK) { std::cerr << "ERROR: twl_comm_init failed (" << rcComm << "): " << twl_last_error() << '\n'; markFailedAtExit(); exit(1); }
        atexit(markFailedAtExit);      // (... and behind RCCL's and the device runtime's handlers, see above)
        if (option.hostStaged) db->ownedPrefix = nullptr;      // (subtree ownership is the device-resident kernel's: --test-fork-host-staged deals and gathers every level)
    };
    const int alnLen = msa::runDefaultAlignment(option, kernel, kernel, rank == 0, [&](msa::SequenceDB *db) { g = msa::progressive::gpu::runTotals(db); }, beforeAlign);
    g_finishedOk = 1;
    if (rank != 0) _exit(0);
    if (watchdog.joinable()) watchdog.join();      // every child has ended well (a bad end leaves from the watchdog)
    const double secs = std::chrono::duration<double>(std::chrono::high_resolution_clock::now() - t0).count();
    std::cerr << "Wrote " << option.outFile << " (length " << alnLen << ") in " << secs << " s; level kernel: " << g.pairs << " pairs, " << g.band_cells
              << " band cells, " << g.relaunched << " pairs re-run in a wider window, " << g.kernel_ms << " ms DP kernel, " << g.total_ms << " ms incl. transfers\n";
    if (option.printDetail)
        std::cerr << "Host phases (ms): prepare " << g.prepare_ms << ", stage " << g.stage_ms << ", boundary call " << g.call_ms << ", finish " << g.finish_ms
                  << "; device prepare kernels " << g.dev_prepare_ms << ", device write-back kernels " << g.dev_commit_ms << '\n';
    return 0;
}
