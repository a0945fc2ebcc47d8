// Step 3's cluster test (BaseCellCalling.step3.py:283-306) over the export of the PASS rows - host code, shared by step3.hip's round
// trip and the host twin (hostio/step3rows.cpp).  The reference string-sorts the PASS rows by (contig text, Start text) - positions
// compare as strings -, tests adjacent pairs on the same contig other than chrM with |p1 - p2| < clust_dist, and tags every row whose
// INDEX text is in the set of those it found.  In: the export's lines, "ordinal \t CHROM:Start:ALT \n" (step3_core.h print_export; no part
// holds a ':').  Out: that set as sorted records (step3_core.h index_record's form), or the row the Python would raise on.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string_view>
#include <vector>
#include "step3_core.h"

namespace lsg3 {

// 0: recs holds the set (n = recs.size() / INDEX_REC).  1: undecided - *bad_ordinal and *reason say which row and why.
inline int cluster_records(const char* text, size_t n_bytes, int64_t clust_dist, std::vector<uint8_t>& recs, int64_t* bad_ordinal, int* reason) {
    using sv = std::string_view;
    struct Entry { sv chrom, pos, index; int64_t ordinal; };
    std::vector<Entry> e;
    const sv all(text, n_bytes);
    for (size_t a = 0; a < all.size();) {
        size_t nl = all.find('\n', a);
        if (nl == sv::npos) nl = all.size();
        const sv line = all.substr(a, nl - a);
        const size_t tab = line.find('\t');
        const sv index = line.substr(tab + 1);
        const size_t c1 = index.find(':'), c2 = index.find(':', c1 + 1);
        int64_t ordinal = 0;
        parse_uint(line.data(), (int)tab, ordinal);
        e.push_back(Entry{index.substr(0, c1), index.substr(c1 + 1, c2 - c1 - 1), index, ordinal});
        a = nl + 1;
    }
    std::stable_sort(e.begin(), e.end(), [](const Entry& x, const Entry& y) { return x.chrom != y.chrom ? x.chrom < y.chrom : x.pos < y.pos; });
    std::vector<const Entry*> trash;
    for (size_t i = 0; i + 1 < e.size(); ++i) {
        if (e[i].chrom != e[i + 1].chrom || e[i].chrom == "chrM") continue;
        int64_t p1, p2;                                  // int(p1), int(p2): what is not a plain integer is left to the Python
        for (const Entry* x : {&e[i], &e[i + 1]})
            if (!parse_uint(x->pos.data(), (int)x->pos.size(), x == &e[i] ? p1 : p2)) { *bad_ordinal = x->ordinal; *reason = LSG_STEP3_POSITION; return 1; }
        if (std::llabs(p1 - p2) < clust_dist) { trash.push_back(&e[i]); trash.push_back(&e[i + 1]); }
    }
    std::vector<std::vector<uint8_t>> one;
    for (const Entry* x : trash) {
        if (x->index.size() > (size_t)LSG_STEP3_INDEX_MAX) { *bad_ordinal = x->ordinal; *reason = LSG_STEP3_INDEX_LONG; return 1; }
        std::vector<uint8_t> r((size_t)INDEX_REC, 0);
        r[0] = (uint8_t)x->index.size();
        memcpy(r.data() + 1, x->index.data(), x->index.size());
        one.push_back(std::move(r));
    }
    std::sort(one.begin(), one.end(), [](const std::vector<uint8_t>& x, const std::vector<uint8_t>& y) { return record_cmp(x.data(), y.data()) < 0; });
    one.erase(std::unique(one.begin(), one.end()), one.end());
    recs.clear();
    for (const auto& r : one) recs.insert(recs.end(), r.begin(), r.end());
    return 0;
}

} // namespace lsg3
