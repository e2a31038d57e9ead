// twilight_amd/csrc/twl_keep_plan.inc.hip -- what the calls of include/twl_keep.h decide on the host, as PURE functions of the call's arguments and of
// the placement's bookkeeping: everything twl_place_finish_keep / twl_place_dropped_counts / twl_place_dropped_runs reject (and what twl_place_finish
// rejects behind a finish_keep), and the tables the runs kernel reads.  No HIP call and no global in this file: tests/keep_plan_kats.cpp includes it
// directly.  Included by twl_place.inc.hip (one translation unit).
#pragma once
#include <cstdint>
#include <unordered_set>
#include <vector>
#include "twl_place_plan.inc.hip"

// What a placement knows once twl_place_finish_keep has run.
struct KeepBook {
    bool done = false;
    std::vector<int32_t> runs, letters;     // per store sequence: dropped runs and letters (collected sequences only)
};

// Everything twl_place_finish_keep rejects: the message, or nullptr.
inline const char *check_keep_finish(const PlaceBook &b, const KeepBook &k, bool haveOuts, int32_t n_seqs, const int32_t *row_len)
{
    if (!haveOuts) return "bad argument";
    if (k.done) return "twl_place_finish_keep called twice";
    if (b.finished) return "twl_place_finish_keep after twl_place_finish";
    for (int32_t id : b.placed)
        if (id < 0 || id >= n_seqs || row_len[id] != b.qlen[id]) return "a placed sequence's row has been rewritten since it was collected";
    return nullptr;
}

// twl_place_finish behind a finish_keep: the message, or nullptr.
inline const char *check_finish_after_keep(const KeepBook &k) { return k.done ? "twl_place_finish after twl_place_finish_keep" : nullptr; }

// After the rows kernel: runs[t] / letters[t] of collected sequence b.placed[t].  The placement is over (nothing can be collected or finished
// any more); *runsTotal / *lettersTotal receive the sums.
inline void keep_finish_done(PlaceBook &b, KeepBook &k, const int32_t *runs, const int32_t *letters, int64_t *runsTotal, int64_t *lettersTotal)
{
    k.runs.assign(b.plen.size(), 0);
    k.letters.assign(b.plen.size(), 0);
    int64_t r = 0, l = 0;
    for (size_t t = 0; t < b.placed.size(); ++t) {
        k.runs[b.placed[t]] = runs[t];
        k.letters[b.placed[t]] = letters[t];
        r += runs[t]; l += letters[t];
    }
    k.done = true;
    b.finished = true;
    *runsTotal = r; *lettersTotal = l;
}

// What both dropped_* calls reject of their list: the message, or nullptr.  `what`: the call's own text for a call before finish_keep.
inline const char *check_keep_ids(const PlaceBook &b, const KeepBook &k, int32_t n, const int32_t *seq_ids, bool haveOuts, const char *what)
{
    if (n < 0 || (n > 0 && (!seq_ids || !haveOuts))) return "bad argument";
    if (!k.done) return what;
    std::unordered_set<int32_t> seen;
    for (int32_t i = 0; i < n; ++i) {
        const int32_t id = seq_ids[i];
        if (id < 0 || id >= (int32_t)b.plen.size()) return "sequence id out of range";
        if (b.plen[id] < 0) return "the sequence was not collected";
        if (!seen.insert(id).second) return "a sequence id is listed twice";
    }
    return nullptr;
}

inline const char *check_dropped_counts(const PlaceBook &b, const KeepBook &k, int32_t n, const int32_t *seq_ids, bool haveOuts)
{
    return check_keep_ids(b, k, n, seq_ids, haveOuts, "twl_place_dropped_counts before twl_place_finish_keep");
}

struct KeepRunsPlan {
    std::vector<int64_t> pathOff, runOff;   // per listed sequence: its path in the arena, its first record
    std::vector<int32_t> plen, nRuns;       // ... its path length, its records
    int64_t total = 0;                      // records of the call
};

// Everything twl_place_dropped_runs rejects: the message, or nullptr with `p` filled in.
inline const char *check_dropped_runs(const PlaceBook &b, const KeepBook &k, int32_t n, const int32_t *seq_ids, const int64_t *run_off, bool haveOuts, KeepRunsPlan &p)
{
    p = KeepRunsPlan{};
    if (const char *why = check_keep_ids(b, k, n, seq_ids, haveOuts && run_off, "twl_place_dropped_runs before twl_place_finish_keep")) return why;
    if (n == 0) return nullptr;
    int64_t at = 0;
    for (int32_t i = 0; i < n; ++i) {
        if (run_off[i] != at) return "run_off is not the exclusive scan of the dropped-run counts";
        const int32_t id = seq_ids[i];
        p.pathOff.push_back(b.slot[id]); p.runOff.push_back(at); p.plen.push_back(b.plen[id]); p.nRuns.push_back(k.runs[id]);
        at += k.runs[id];
    }
    if (run_off[n] != at) return "run_off is not the exclusive scan of the dropped-run counts";
    p.total = at;
    return nullptr;
}
