// lsio_build_bai_full (hostio/bamio.cpp, bamindex_core.h) under a sanitizer, on the CPU: the BAM named on the command line and its
// truncations - every length around each BGZF member's edges and a stride through the rest.  Every call must return (0 or an
// error), read nothing outside the file and leak nothing; the whole file must index, and a truncation must never give the whole file's index.
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined tests/native/bai_full_check.cpp longsom_amd/csrc/hostio/bamio.cpp -lz -pthread -o bai_full_check
//   ./bai_full_check some.bam /tmp/workdir
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <string>
#include <vector>

extern "C" {
int lsio_build_bai_full(const char*, const char*);
int lsio_build_bai_full_info(const char*, const char*, int64_t*);
const char* lsio_last_error(void);
}

static std::vector<uint8_t> slurp(const std::string& p) {
    std::vector<uint8_t> v;
    FILE* f = fopen(p.c_str(), "rb");
    if (!f) return v;
    uint8_t buf[65536]; size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + n);
    fclose(f);
    return v;
}

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage: %s file.bam workdir\n", argv[0]); return 2; }
    const std::string work = argv[2], cut = work + "/cut.bam", bai = work + "/cut.bam.bai";
    const std::vector<uint8_t> raw = slurp(argv[1]);
    if (raw.size() < 28) { fprintf(stderr, "%s: not read\n", argv[1]); return 2; }
    int64_t info[10];
    if (lsio_build_bai_full_info(argv[1], bai.c_str(), info) != 0) { fprintf(stderr, "the whole file: %s\n", lsio_last_error()); return 1; }
    const std::vector<uint8_t> whole = slurp(bai);
    if ((int64_t)whole.size() != info[7]) { fprintf(stderr, "the index has %zu bytes, info says %lld\n", whole.size(), (long long)info[7]); return 1; }
    std::set<size_t> lens;
    for (size_t off = 0; off + 18 <= raw.size();) {            // the members' edges (a BC subfield first in the extra field, as every writer here puts it)
        const size_t bsize = (size_t)(raw[off + 16] | (raw[off + 17] << 8)) + 1;
        for (long d = -9; d <= 19; ++d) { const long x = (long)off + d; if (x >= 0 && (size_t)x < raw.size()) lens.insert((size_t)x); }
        off += bsize;
    }
    const size_t stride = raw.size() / 400 + 1;
    for (size_t n = 0; n < raw.size(); n += stride) lens.insert(n);
    int ok = 0, refused = 0;
    for (size_t n : lens) {
        FILE* f = fopen(cut.c_str(), "wb");
        if (!f || fwrite(raw.data(), 1, n, f) != n) { fprintf(stderr, "cannot write %s\n", cut.c_str()); return 2; }
        fclose(f);
        remove(bai.c_str());
        if (lsio_build_bai_full(cut.c_str(), bai.c_str()) == 0) {
            ++ok;
            if (slurp(bai) == whole && n + 28 < raw.size() && info[0] > 0) { fprintf(stderr, "%zu of %zu bytes give the whole file's index\n", n, raw.size()); return 1; }
        } else ++refused;
    }
    printf("%s: %lld records, index of %zu bytes; %zu truncations: %d indexed (cut on a member's edge), %d refused\n", argv[1], (long long)info[0], whole.size(), lens.size(), ok, refused);
    return 0;
}
