// jpeglibrary_amd/csrc/device_optimize.cpp -- JpegOptimizer (ref: JpegOptimizer.cs) for a batch of baseline files.
//
// The reference runs two passes over one file: Scan() decodes every symbol of the scan and counts it per Huffman table
// (:360-463), builds new tables from the counts (JpegHuffmanEncodingTableBuilder.Build), and Optimize() walks the file
// again, copying the segments it keeps, writing the new DHT in place of the first one and re-writing the scan symbol by
// symbol with the new codes (:540-880).  Here the marker walks run on the host (they touch a few hundred bytes), the
// symbol passes on the GPU: K1 (marker index + unstuffing, shared with the decoder) then KT count -> host table build ->
// KT measure -> exclusive scan -> KT emit (kt_transcode.hip).  The output is assembled from the host pieces and the
// device-resident scan data at download time.
//
// Fences (reported as JPGPU_ERR_NOT_SUPPORTED): files with more than one scan (the reference builds its tables from the
// LAST scan only, :462, and then fails or writes garbage for the others), progressive frames (:580-582), a restart interval
// that changes between the frame header and the scan or after the scan.  Parity of the bytes is unpinned (the reference holds no golden bytes, and
// .NET's unstable sort decides the order of equal-length symbols in the DHT).
#include "device_optimize.h"
#include "device_encode.h"

#include <algorithm>
#include <cstring>
#include <map>
#include <utility>

namespace jpgpu {

// ------------------------------------------------------------------------------------------------ table builder
namespace {
struct Sym {
    int64_t frequency;
    int16_t value;
    uint16_t code_size;
    int16_t others;
};

// Array.Sort(T[], Comparison<T>) / List<T>.Sort(Comparison<T>) of .NET Core 3.0+ / .NET 5+ (ArraySortHelper<T>.IntrospectiveSort:
// insertion sort up to 16 elements, median-of-three pivot parked at hi - 1, heapsort below depth 2 * (log2(n) + 1)).  The
// reference orders its symbols and its package-merge nodes with it, and the sort is not stable: what it leaves depends on
// the algorithm, so the algorithm is restated.  It only moves whole elements and looks at them through the comparison,
// which makes an array of pointers to the elements take exactly the same path.
template <typename T, typename Cmp>
struct NetSort {
    const T **k;
    Cmp cmp;
    void swap_if_greater(int i, int j) {
        if (i != j && cmp(*k[i], *k[j]) > 0) std::swap(k[i], k[j]);
    }
    void insertion(int lo, int n) {
        for (int i = 0; i < n - 1; i++) {
            const T *t = k[lo + i + 1];
            int j = i;
            while (j >= 0 && cmp(*t, *k[lo + j]) < 0) {
                k[lo + j + 1] = k[lo + j];
                j--;
            }
            k[lo + j + 1] = t;
        }
    }
    void down_heap(int lo, int i, int n) {
        const T *d = k[lo + i - 1];
        while (i <= n >> 1) {
            int child = 2 * i;
            if (child < n && cmp(*k[lo + child - 1], *k[lo + child]) < 0) child++;
            if (!(cmp(*d, *k[lo + child - 1]) < 0)) break;
            k[lo + i - 1] = k[lo + child - 1];
            i = child;
        }
        k[lo + i - 1] = d;
    }
    void heap(int lo, int n) {
        for (int i = n >> 1; i >= 1; i--) down_heap(lo, i, n);
        for (int i = n; i > 1; i--) {
            std::swap(k[lo], k[lo + i - 1]);
            down_heap(lo, 1, i - 1);
        }
    }
    int partition(int lo, int n) {
        const int hi = n - 1, middle = hi >> 1;
        swap_if_greater(lo, lo + middle);
        swap_if_greater(lo, lo + hi);
        swap_if_greater(lo + middle, lo + hi);
        const T *pivot = k[lo + middle];
        std::swap(k[lo + middle], k[lo + hi - 1]);
        int left = 0, right = hi - 1;
        while (left < right) {
            while (cmp(*k[lo + ++left], *pivot) < 0) {
            }
            while (cmp(*pivot, *k[lo + --right]) < 0) {
            }
            if (left >= right) break;
            std::swap(k[lo + left], k[lo + right]);
        }
        if (left != hi - 1) std::swap(k[lo + left], k[lo + hi - 1]);
        return left;
    }
    void intro(int lo, int n, int depth) {
        while (n > 1) {
            if (n <= 16) {
                if (n == 2) {
                    swap_if_greater(lo, lo + 1);
                } else if (n == 3) {
                    swap_if_greater(lo, lo + 1);
                    swap_if_greater(lo, lo + 2);
                    swap_if_greater(lo + 1, lo + 2);
                } else {
                    insertion(lo, n);
                }
                return;
            }
            if (depth == 0) {
                heap(lo, n);
                return;
            }
            depth--;
            const int p = partition(lo, n);
            intro(lo + p + 1, n - (p + 1), depth);
            n = p;
        }
    }
};
template <typename T, typename Cmp>
void net_sort(std::vector<const T *> &ptrs, Cmp cmp) {
    const int n = (int)ptrs.size();
    if (n < 2) return;
    int log2 = 0;
    for (unsigned v = (unsigned)n; v > 1; v >>= 1) log2++;
    NetSort<T, Cmp> s{ptrs.data(), cmp};
    s.intro(0, n, 2 * (log2 + 1));
}
template <typename Cmp>
void net_sort_symbols(Sym *s, int n, Cmp cmp) {
    std::vector<Sym> copy(s, s + n);
    std::vector<const Sym *> ptrs((size_t)n);
    for (int i = 0; i < n; i++) ptrs[i] = &copy[i];
    net_sort<Sym>(ptrs, cmp);
    for (int i = 0; i < n; i++) s[i] = *ptrs[i];
}

// BuildCanonicalCode: code words for lengths already in DHT order (:237-283, :470-497)
void assign_canonical_codes(std::vector<OptimalCode> &codes) {
    uint16_t code = 0;
    int count = codes[0].length;
    codes[0].code = 0;
    for (size_t i = 1; i < codes.size(); i++) {
        OptimalCode &c = codes[i];
        if (c.length > count) {
            code++;
            code = (uint16_t)(code << (c.length - count));
            c.code = code;
            count = c.length;
        } else {
            c.code = ++code;
        }
    }
}

// MostOptimalCoding: BuildUsingPackageMerge + RunPackageMerge (JpegHuffmanEncodingTableBuilder.cs:289-428)
struct PmNode {
    int64_t frequency = 0;
    int16_t index = 0;
    const PmNode *left = nullptr, *right = nullptr;
};
void pm_traverse(const PmNode *node, Sym *symbols) {
    if (!node) return;
    if (!node->left) {
        symbols[node->index].code_size++;
    } else {
        pm_traverse(node->left, symbols);
        pm_traverse(node->right, symbols);
    }
}
bool build_package_merge(const uint32_t freq[256], std::vector<OptimalCode> *codes) {
    int code_count = 0;
    for (int i = 0; i < 256; i++) code_count += freq[i] != 0;
    if (code_count == 0) return false;
    Sym s[257];
    int n = 0;
    for (int i = 0; i < 256; i++)
        if (freq[i] != 0) s[n++] = {(int64_t)freq[i], (int16_t)i, 0, 0};
    s[n++] = {0, -1, 0, 0};
    net_sort_symbols(s, n, [](const Sym &x, const Sym &y) { return y.frequency < x.frequency ? -1 : (y.frequency > x.frequency ? 1 : 0); });
    std::vector<PmNode> pool;
    pool.reserve((size_t)n * 40);
    std::vector<const PmNode *> levels[16];
    for (int l = 15; l >= 0; l--)
        for (int i = 0; i < n; i++) {
            pool.push_back(PmNode{s[i].frequency, (int16_t)i, nullptr, nullptr});
            levels[l].push_back(&pool.back());
        }
    auto desc = [](const PmNode &x, const PmNode &y) { return y.frequency < x.frequency ? -1 : (y.frequency > x.frequency ? 1 : 0); };
    auto asc = [](const PmNode &x, const PmNode &y) { return x.frequency < y.frequency ? -1 : (x.frequency > y.frequency ? 1 : 0); };
    for (int l = 15; l > 0; l--) {
        std::vector<const PmNode *> &nodes = levels[l];
        net_sort<PmNode>(nodes, desc);
        while (nodes.size() >= 2) {
            const PmNode *n1 = nodes[nodes.size() - 1], *n2 = nodes[nodes.size() - 2];
            nodes.resize(nodes.size() - 2);
            pool.push_back(PmNode{n1->frequency + n2->frequency, 0, n1, n2});
            levels[l - 1].push_back(&pool.back());
        }
    }
    net_sort<PmNode>(levels[0], asc);
    const int select = std::max(1, 2 * (n - 1));
    for (int i = 0; i < select; i++) pm_traverse(levels[0][(size_t)i], s);
    net_sort_symbols(s, n, [](const Sym &x, const Sym &y) {  // SymbolComparer (:430-453)
        if (x.code_size > y.code_size) return 1;
        if (x.code_size < y.code_size) return -1;
        if (x.frequency > y.frequency) return -1;
        if (x.frequency < y.frequency) return 1;
        return 0;
    });
    int index = 0;
    for (int i = n - 1; i >= 0; i--)
        if (s[i].value == -1) {
            index = i;
            break;
        }
    for (int i = index; i < n - 1; i++) s[i] = s[i + 1];
    codes->assign((size_t)code_count, OptimalCode{0, 0, 0});
    for (int i = 0; i < code_count; i++) {
        if (s[i].code_size > 16) return false;
        (*codes)[i].symbol = (uint8_t)s[i].value;
        (*codes)[i].length = (uint8_t)s[i].code_size;
    }
    assign_canonical_codes(*codes);
    return true;
}
}  // namespace

void net_sort_permutation(const int32_t *keys, int n, int32_t *perm) {
    std::vector<const int32_t *> ptrs((size_t)std::max(0, n));
    for (int i = 0; i < n; i++) ptrs[(size_t)i] = keys + i;
    net_sort<int32_t>(ptrs, [](const int32_t &x, const int32_t &y) { return x < y ? -1 : (x > y ? 1 : 0); });
    for (int i = 0; i < n; i++) perm[i] = (int32_t)(ptrs[(size_t)i] - keys);
}

bool build_optimal_table(const uint32_t freq[256], std::vector<OptimalCode> *codes, bool most_optimal) {
    if (most_optimal) return build_package_merge(freq, codes);
    int code_count = 0;
    for (int i = 0; i < 256; i++) code_count += freq[i] != 0;
    if (code_count == 0) return false;
    Sym s[257];
    int n = 0;
    for (int i = 0; i < 256; i++)
        if (freq[i] != 0) s[n++] = {(int64_t)freq[i], (int16_t)i, 0, -1};
    s[n++] = {1, -1, 0, -1};  // the reserved symbol that keeps the all-ones code unused
    // Figure K.1 as the reference runs it (:178-235): least frequency, FIRST index among equals
    for (;;) {
        int v1 = -1, v2 = -1;
        int64_t f1 = -1, f2 = -1;
        for (int i = 0; i < n; i++)
            if (s[i].frequency >= 0 && (v1 == -1 || s[i].frequency < f1)) {
                v1 = i;
                f1 = s[i].frequency;
            }
        for (int i = 0; i < n; i++)
            if (s[i].frequency >= 0 && i != v1 && (v2 == -1 || s[i].frequency < f2)) {
                v2 = i;
                f2 = s[i].frequency;
            }
        if (v2 == -1) break;
        s[v1].frequency += s[v2].frequency;
        s[v2].frequency = -1;
        s[v1].code_size++;
        while (s[v1].others != -1) {
            v1 = s[v1].others;
            s[v1].code_size++;
        }
        s[v1].others = (int16_t)v2;
        s[v2].code_size++;
        while (s[v2].others != -1) {
            v2 = s[v2].others;
            s[v2].code_size++;
        }
    }
    // Figures K.2 / K.3 on the reference's 0-based 60-entry byte array (:117-158)
    uint8_t bits[60] = {};
    int index = 32;
    for (int i = 0; i < n; i++) {
        const int cs = s[i].code_size;
        if (cs > 0) {
            index = std::max(index, cs);
            if (index >= 60) return false;
            bits[cs - 1]++;
        }
    }
    // The counters are BYTES in the reference (Span<byte> bits, :118): 256 codes of one length -- 255 symbols of nearly equal
    // frequency plus the reserved one, a perfect tree of depth 8 -- wrap to zero, and the searches below then walk off the
    // front of the span: the reference throws IndexOutOfRangeException.  Same here: failure, not a walk through the stack.
    for (;;) {
        while (bits[index] > 0) {
            int j = index - 1;
            do {
                j -= 1;
                if (j < 0) return false;
            } while (bits[j] == 0);
            bits[index] = (uint8_t)(bits[index] - 2);
            bits[index - 1] = (uint8_t)(bits[index - 1] + 1);
            bits[j + 1] = (uint8_t)(bits[j + 1] + 2);
            bits[j] = (uint8_t)(bits[j] - 1);
        }
        index -= 1;
        if (index != 15) continue;
        while (bits[index] == 0) {
            index--;
            if (index < 0) return false;
        }
        bits[index]--;
        break;
    }
    for (int i = 0; i < n; i++)
        if (s[i].value == -1) s[i].code_size = 0xFFFF;
    net_sort_symbols(s, n, [](const Sym &x, const Sym &y) { return x.code_size < y.code_size ? -1 : (x.code_size > y.code_size ? 1 : 0); });
    // BuildCanonicalCode (:237-283)
    codes->assign((size_t)code_count, OptimalCode{0, 0, 0});
    int length = 1, at = 0;
    uint8_t left = bits[0];
    for (int i = 0; i < code_count; i++) {
        while (left == 0) {
            left = bits[++at];
            length++;
        }
        left--;
        (*codes)[i].symbol = (uint8_t)s[i].value;
        (*codes)[i].length = (uint8_t)length;
    }
    assign_canonical_codes(*codes);
    return true;
}

void optimal_codes_to_table(const std::vector<OptimalCode> &codes, EncHuffTable *table, std::vector<uint8_t> *dht) {
    for (int sym = 0; sym < 256; sym++) {
        table->code[sym] = codes[0].code;
        table->len[sym] = codes[0].length;
    }
    for (const OptimalCode &c : codes) {
        table->code[c.symbol] = c.code;
        table->len[c.symbol] = c.length;
    }
    for (int l = 1; l <= 16; l++) {
        int count = 0;
        for (const OptimalCode &c : codes) count += c.length == l;
        dht->push_back((uint8_t)count);
    }
    for (const OptimalCode &c : codes) dht->push_back(c.symbol);
}

// ------------------------------------------------------------------------------------------------ batch
void OptimizeBatch::Road::release() {
    batch.reset();
    for (DevBuffer *b : {&d_turn_images, &d_turn_work, &d_coefs, &d_images, &d_layouts, &d_work_blk, &d_work_stat, &d_hist, &d_tables}) b->release();
    tail.release();
}

OptimizeBatch::~OptimizeBatch() {
    for (DevBuffer *b : {&d_work_, &d_scan_ids_, &d_hist_, &d_enc_, &d_sizes_, &d_offsets_, &d_base_, &d_totals_, &d_out_, &d_sub_work_,
                         &d_sub_scan_ids_, &d_sub_bits_, &d_sub_bitoff_, &d_sub_totals_, &d_scan_raw_off_, &d_raw_, &d_simages_, &d_swork_chunk_,
                         &d_chunk_ff_, &d_sout_, &d_sout_len_})
        b->release();
    road_.release();
    for (hipEvent_t ev : {ev0_, ev1_, road_.ev_kx[0], road_.ev_kx[1], road_.ev_td[0], road_.ev_td[1], road_.ev_td[2]})
        if (ev) (void)hipEventDestroy(ev);
}
int OptimizeBatch::fail(int status, const std::string &msg) {
    ctx_->last_error = msg;
    return status;
}
int OptimizeBatch::hip_fail(hipError_t e, const char *what) {
    return fail(JPGPU_ERR_DEVICE, std::string(what) + ": " + hipGetErrorString(e));
}

// what upload()'s stages hand one another
struct OptimizeBatch::Upload {
    const uint8_t *const *jpeg;
    const size_t *len;
    int n;
    bool strip;
    std::vector<uint8_t> given;       // the orientations of THIS upload (empty: every image by the policy)
    std::vector<jpgpu_rect> windows;  // ... and its windows (empty: none)
    std::vector<int> turned;          // the images that take the coefficient road, in order
};

int OptimizeBatch::upload(const uint8_t *const *jpeg, const size_t *len, int n, int strip) {
    if (n < 0 || (n > 0 && (!jpeg || !len))) return fail(JPGPU_ERR_ARGUMENT, "jpgpu_optimizer_upload: bad arguments");
    plans_.clear();
    ran_ = false;
    Upload u{jpeg, len, n, strip != 0, {}, {}, {}};
    int rc = take_pending_lists(u);
    if (rc != JPGPU_OK) return rc;
    plans_.assign((size_t)n, Plan());
    plan_on_host(u);
    if ((rc = hand_files_to_decoder(u)) != JPGPU_OK) return rc;
    admit_and_sort(u);
    if ((rc = plan_road(u)) != JPGPU_OK) return rc;
    return reserve_and_upload();
}

int OptimizeBatch::take_pending_lists(Upload &u) {
    u.given.swap(pending_orientations_);
    u.windows.swap(pending_windows_);
    if (!u.given.empty() && (int)u.given.size() != u.n)
        return fail(JPGPU_ERR_ARGUMENT, "jpgpu_optimizer_upload: the upload's n differs from the orientations' n (jpgpu_optimizer_set_orientations)");
    if (!u.windows.empty() && (int)u.windows.size() != u.n)
        return fail(JPGPU_ERR_ARGUMENT, "jpgpu_optimizer_upload: the upload's n differs from the windows' n (jpgpu_optimizer_set_windows)");
    return JPGPU_OK;
}

// the marker walks (optimize_walk.h), the plan of the lossless transform, the swallowed-terminator verdict
void OptimizeBatch::plan_on_host(const Upload &u) {
    for (int i = 0; i < u.n; i++) {
        Plan &p = plans_[(size_t)i];
        ScanEndCache ends;
        try {
            walk_file(p, ends, u.jpeg[i], u.len[i], u.strip);
            plan_turned_image(p, u.jpeg[i], u.len[i], u.strip, u.given.empty() ? 0 : u.given[(size_t)i], u.windows.empty() ? nullptr : &u.windows[(size_t)i]);
        } catch (const Refuse &e) {
            p.refused(e);
        }
        if (p.status == JPGPU_OK) walk_swallowed_terminator(p, ends, u.jpeg[i], u.len[i], u.strip);
    }
}

// the decoder-side parser resolves the scan (tables, geometry, restart interval) and lays the files out in HBM
int OptimizeBatch::hand_files_to_decoder(const Upload &u) {
    batch_.set_entropy_only(true);
    std::vector<int> dri((size_t)u.n, 0);
    std::vector<uint8_t> no_subseq((size_t)u.n, 0);
    for (int i = 0; i < u.n; i++) {
        dri[i] = plans_[i].dri_at_scan;
        no_subseq[i] = plans_[i].rsts_in_scan != 0;  // RSTn behind the last block: the interval kernel knows what to do
    }
    batch_.set_preset_restart_intervals(std::move(dri));
    batch_.set_preset_no_subseq(std::move(no_subseq));
    return batch_.upload_files(u.jpeg, u.len, u.n, JPGPU_FMT_PLANAR_U8);
}

// what the decoder-side batch made of each file decides whether the image is taken, and which kernels transcode it
void OptimizeBatch::admit_and_sort(Upload &u) {
    scan_ids_.clear();
    work_.clear();
    sub_scan_ids_.clear();
    sub_work_.clear();
    // the images of the coefficient road: Scan()'s pass decides their status, nothing of it is emitted
    std::vector<HuffWork> counted_only, sub_counted_only;
    const auto refuse_image = [](Plan &p, const char *msg) {
        p.status = JPGPU_ERR_NOT_SUPPORTED;
        p.detail = kDetailUnsupportedFrame;
        p.error = msg;
        p.job = -1;
    };
    for (int i = 0; i < u.n; i++) {
        Plan &p = plans_[i];
        if (p.status != JPGPU_OK) continue;
        const ImagePlan *img = batch_.image(i);
        if (img->status != JPGPU_OK) {
            static_cast<Verdict &>(p) = {img->status, img->detail, img->error};
            continue;
        }
        if (img->jobs.size() != 1 || batch_.jobs_[img->jobs[0]].kind != kScanSequential) {
            refuse_image(p, "Only single-scan baseline files are supported by the optimizer path.");
            continue;
        }
        p.job = img->jobs[0];
        const DevScan &s = batch_.h_scans_[p.job];
        if ((int)s.dri != p.dri_at_scan) {  // a DRI segment in front of the frame header that a later one overrides
            refuse_image(p, "A restart interval that changes between the frame header and the scan is not supported by the optimizer path.");
            continue;
        }
        p.by_subsequence = s.n_subs != 0;  // the batch marks DRI = 0 scans for the self-synchronising subsequence machinery
                                           // (not those with RSTn markers in the data: upload() asks for the interval path)
        const bool turned = p.transform.coefficient_road();
        if (turned) {
            u.turned.push_back(i);
        } else {  // (jpgpu_optimizer_image_transform: the frame as it is)
            const ScanJob &job = batch_.jobs_[p.job];
            p.transform.out_width = img->width;
            p.transform.out_height = img->height;
            p.transform.ncomp = std::min<int>(4, (int)job.geo.frame.components.size());
            for (int c = 0; c < p.transform.ncomp; c++) {
                p.transform.h[c] = job.geo.frame.components[(size_t)c].h;
                p.transform.v[c] = job.geo.frame.components[(size_t)c].v;
            }
        }
        if (p.by_subsequence) {
            if (!turned) sub_scan_ids_.push_back((uint32_t)p.job);
            for (uint32_t first = 0; first < s.n_subs; first += 256) (turned ? sub_counted_only : sub_work_).push_back({(uint32_t)p.job, first});
        } else {
            if (!turned) scan_ids_.push_back((uint32_t)p.job);
            for (uint32_t first = 0; first < s.n_intervals; first += 256) (turned ? counted_only : work_).push_back({(uint32_t)p.job, first});
        }
    }
    n_work_emit_ = (int)work_.size();
    n_sub_work_emit_ = (int)sub_work_.size();
    work_.insert(work_.end(), counted_only.begin(), counted_only.end());
    sub_work_.insert(sub_work_.end(), sub_counted_only.begin(), sub_counted_only.end());
}

int OptimizeBatch::reserve_and_upload() {
    const size_t n_jobs = batch_.h_scans_.size();
    const DevUpload ups[] = {
        {&d_work_, work_.data(), work_.size() * sizeof(HuffWork), 0},
        {&d_scan_ids_, scan_ids_.data(), scan_ids_.size() * sizeof(uint32_t), 0},
        {&d_hist_, nullptr, 0, n_jobs * kMaxHuffSlots * 256 * sizeof(uint32_t) + 256},
        {&d_enc_, nullptr, 0, n_jobs * kMaxHuffSlots * sizeof(EncHuffTable) + 256},
        {&d_sizes_, nullptr, 0, (size_t)batch_.total_ends_ * sizeof(uint32_t) + 256},
        {&d_offsets_, nullptr, 0, (size_t)batch_.total_ends_ * sizeof(uint64_t) + 256},
        {&d_base_, nullptr, 0, scan_ids_.size() * sizeof(uint64_t) + 256},
        {&d_totals_, nullptr, 0, scan_ids_.size() * sizeof(uint64_t) + 256},
        {&d_sub_work_, sub_work_.data(), sub_work_.size() * sizeof(HuffWork), 0},
        {&d_sub_scan_ids_, sub_scan_ids_.data(), sub_scan_ids_.size() * sizeof(uint32_t), 0},
        {&d_sub_bits_, nullptr, 0, (size_t)batch_.total_subs_ * sizeof(uint32_t) + 256},
        {&d_sub_bitoff_, nullptr, 0, (size_t)batch_.total_subs_ * sizeof(uint64_t) + 256},
        {&d_sub_totals_, nullptr, 0, sub_scan_ids_.size() * sizeof(uint64_t) + 256},
        {&d_scan_raw_off_, nullptr, 0, n_jobs * sizeof(uint64_t) + 256},
        {&d_simages_, nullptr, 0, sub_scan_ids_.size() * sizeof(DevEncImage) + 256},
        {&d_sout_len_, nullptr, 0, sub_scan_ids_.size() * sizeof(uint64_t) + 256},
    };
    bool copying = false;
    const hipError_t e = reserve_and_copy(ups, ctx_->stream, &copying);
    return e == hipSuccess ? JPGPU_OK : hip_fail(e, copying ? "hipMemcpyAsync(optimizer work)" : "hipMalloc");
}

// what run()'s stages hand one another
struct OptimizeBatch::Run {
    size_t n_jobs = 0;
    int n_work = 0, n_scans = 0, n_sub_work = 0, n_sub_scans = 0, n_slots = 0;  // (work: what is measured and emitted ...
    int n_work_counted = 0, n_sub_work_counted = 0;                             // ... and what is counted: the turned images' too)
    int n_turned = 0;
    const int16_t *turn_src = nullptr;  // the dense store of road_.batch
    const uint8_t *udata = nullptr, *input = nullptr;
    const DevScan *scans = nullptr;
    DevScanStatus *status = nullptr;
    const DevHuffTable *pool = nullptr;
    const uint32_t *ends_u = nullptr, *ends_raw = nullptr;
    const uint32_t *exit_state = nullptr, *first_block = nullptr;  // of the subsequence synchronisation
    std::vector<uint64_t> totals, base;                            // per interval scan: bytes, place in d_out_
    std::vector<uint64_t> sub_total_bits, sout_len;                // per subsequence scan: raw bits, stuffed bytes
    std::vector<DevEncImage> simages;                              // ... and its descriptor for the stuffing stage
};

int OptimizeBatch::run() {
    ran_ = false;
    for (hipEvent_t *ev : {&ev0_, &ev1_, &road_.ev_kx[0], &road_.ev_kx[1], &road_.ev_td[0], &road_.ev_td[1], &road_.ev_td[2]})
        if (!*ev && hipEventCreate(ev) != hipSuccess) return fail(JPGPU_ERR_DEVICE, "hipEventCreate");
    (void)hipEventRecord(ev0_, ctx_->stream);
    int rc = batch_.run_marker_index();
    if (rc != JPGPU_OK) return rc;
    Run r;
    r.n_jobs = batch_.h_scans_.size();
    r.n_work = n_work_emit_;
    r.n_work_counted = (int)work_.size();
    r.n_scans = (int)scan_ids_.size();
    r.n_sub_work = n_sub_work_emit_;
    r.n_sub_work_counted = (int)sub_work_.size();
    r.n_turned = (int)road_.images.size();
    road_.ms[0] = road_.ms[1] = road_.ms[2] = 0;
    r.n_sub_scans = (int)sub_scan_ids_.size();
    r.n_slots = batch_.n_huff_slots_;
    r.udata = (const uint8_t *)batch_.d_unstuffed_.ptr;
    r.input = (const uint8_t *)batch_.d_input_.ptr;
    r.scans = (const DevScan *)batch_.d_scans_.ptr;
    r.status = (DevScanStatus *)batch_.d_status_.ptr;
    r.pool = (const DevHuffTable *)batch_.d_huff_pool_.ptr;
    r.ends_u = (const uint32_t *)batch_.d_ends_u_.ptr;
    r.ends_raw = (const uint32_t *)batch_.d_ends_.ptr;
    if ((rc = count_symbols(r)) != JPGPU_OK) return rc;
    if ((rc = build_tables(r)) != JPGPU_OK) return rc;
    if ((rc = measure_and_place(r)) != JPGPU_OK) return rc;
    if ((rc = emit_intervals(r)) != JPGPU_OK) return rc;
    if (r.n_sub_scans && (rc = emit_subsequences_and_stuff(r)) != JPGPU_OK) return rc;
    if (r.n_turned) {
        if ((rc = decode_turned(r)) != JPGPU_OK) return rc;
        if ((rc = turn_blocks(r)) != JPGPU_OK) return rc;
        if ((rc = build_turned_tables(r)) != JPGPU_OK) return rc;
        if ((rc = emit_turned(r)) != JPGPU_OK) return rc;
    }
    (void)hipEventRecord(ev1_, ctx_->stream);
    hipError_t e = hipStreamSynchronize(ctx_->stream);
    if (e != hipSuccess) return hip_fail(e, "hipStreamSynchronize");
    (void)hipEventElapsedTime(&last_ms_, ev0_, ev1_);
    if (r.n_turned) {
        (void)hipEventElapsedTime(&road_.ms[0], road_.ev_kx[0], road_.ev_kx[1]);
        (void)hipEventElapsedTime(&road_.ms[1], road_.ev_td[0], road_.ev_td[1]);
        (void)hipEventElapsedTime(&road_.ms[2], road_.ev_td[1], road_.ev_td[2]);
    }
    collect_lengths(r);
    ran_ = true;
    return JPGPU_OK;
}

// ---- Scan(): IncrementCodeCount for every symbol
int OptimizeBatch::count_symbols(Run &r) {
    hipError_t e = hipMemsetAsync(d_hist_.ptr, 0, r.n_jobs * kMaxHuffSlots * 256 * sizeof(uint32_t), ctx_->stream);
    if (e != hipSuccess) return hip_fail(e, "hipMemsetAsync(histograms)");
    e = launch_transcode(ctx_->stream, 0, r.udata, r.input, r.scans, (const HuffWork *)d_work_.ptr, r.n_work_counted, r.ends_u, r.ends_raw, r.status, r.pool,
                         (uint32_t *)d_hist_.ptr, nullptr, nullptr, nullptr, nullptr, r.n_slots);
    if (e != hipSuccess) return hip_fail(e, "transcode_kernel<count>");
    // scans without restart intervals: the decoder's self-synchronising subsequences, then the same three passes per subsequence
    if (r.n_sub_work_counted) {
        const int rc = batch_.run_subseq_sync(&r.exit_state, &r.first_block);
        if (rc != JPGPU_OK) return rc;
        e = launch_subseq_transcode(ctx_->stream, 0, r.udata, r.scans, (const HuffWork *)d_sub_work_.ptr, r.n_sub_work_counted, r.ends_u, r.status, r.pool, r.exit_state,
                                    r.first_block, (uint32_t *)d_hist_.ptr, nullptr, nullptr, nullptr, nullptr, nullptr, r.n_slots);
        if (e != hipSuccess) return hip_fail(e, "subseq_transcode_kernel<count>");
    }
    h_hist_.assign(r.n_jobs * kMaxHuffSlots * 256, 0);
    e = hipMemcpyAsync(h_hist_.data(), d_hist_.ptr, h_hist_.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx_->stream);
    if (e != hipSuccess) return hip_fail(e, "hipMemcpyAsync(histograms)");
    e = hipStreamSynchronize(ctx_->stream);
    if (e != hipSuccess) return hip_fail(e, "hipStreamSynchronize");
    return JPGPU_OK;
}

// ---- BuildTables (:462) of one image: one table per (class, identifier) in builder-creation order == the job's slot order, and the DHT
// segment they make
void OptimizeBatch::build_image_tables(Plan &p, const uint32_t *hist, EncHuffTable *enc) const {
    const ScanJob &job = batch_.jobs_[p.job];
    std::vector<uint8_t> body;
    for (int t = 0; t < job.n_huff; t++) {
        std::vector<OptimalCode> codes;
        const uint32_t *freq = hist + (size_t)t * 256;
        if (!build_optimal_table(freq, &codes, most_optimal_)) {
            // No symbol counted: a failing scan (reported from the device status below, which comes first), or a component
            // without blocks -- a sampling factor of zero, which JpegOptimizer never divides by -- whose builders stay empty:
            // Build() throws "No symbol is recorded." (tests/golden/stress/optimizer_component_without_blocks_421.jpg).
            // Symbols counted and no table: the reference's byte counters overflowed (build_optimal_table) -- its Build() dies
            // with IndexOutOfRangeException.
            bool any = false;
            for (int sym = 0; sym < 256; sym++) any |= freq[sym] != 0;
            if (!p.build_failed) {  // behind the scan's own failures (BuildTables runs after ProcessScanBaseline, :462), in front of
                                    // what the markers behind the scan throw (`late` as the walk left it); first builder wins
                p.build_failed = true;
                p.late = {JPGPU_ERR_INVALID_OPERATION, 0, any ? "Index was outside the bounds of the array." : "No symbol is recorded."};
            }
            continue;
        }
        // JpegHuffmanEncodingTableCollection.Write (:172-190): Tc/Th, then the table's own bytes
        body.push_back((uint8_t)(job.huff_copy[t].table_class << 4 | (job.huff_copy[t].identifier & 0xF)));
        optimal_codes_to_table(codes, &enc[t], &body);
    }
    p.dht.clear();
    put_marker(p.dht, 0xC4);
    put_length(p.dht, (uint16_t)body.size());
    p.dht.append(body.begin(), body.end());
}

int OptimizeBatch::build_tables(Run &r) {
    std::vector<EncHuffTable> enc(r.n_jobs * kMaxHuffSlots);
    memset(enc.data(), 0, enc.size() * sizeof(EncHuffTable));
    for (Plan &p : plans_)
        if (p.status == JPGPU_OK && p.job >= 0) build_image_tables(p, &h_hist_[(size_t)p.job * kMaxHuffSlots * 256], &enc[(size_t)p.job * kMaxHuffSlots]);
    const hipError_t e = hipMemcpyAsync(d_enc_.ptr, enc.data(), enc.size() * sizeof(EncHuffTable), hipMemcpyHostToDevice, ctx_->stream);
    return e == hipSuccess ? JPGPU_OK : hip_fail(e, "hipMemcpyAsync(encoding tables)");
}

// ---- Optimize(): size of every interval and subsequence, and where the interval scans' bytes go
int OptimizeBatch::measure_and_place(Run &r) {
    hipError_t e = launch_transcode(ctx_->stream, 1, r.udata, r.input, r.scans, (const HuffWork *)d_work_.ptr, r.n_work, r.ends_u, r.ends_raw, r.status, r.pool,
                                    nullptr, (const EncHuffTable *)d_enc_.ptr, (uint32_t *)d_sizes_.ptr, nullptr, nullptr, r.n_slots);
    if (e != hipSuccess) return hip_fail(e, "transcode_kernel<measure>");
    e = launch_transcode_offsets(ctx_->stream, r.scans, (const uint32_t *)d_scan_ids_.ptr, r.n_scans, (const uint32_t *)d_sizes_.ptr, nullptr, nullptr,
                                 (uint64_t *)d_totals_.ptr);
    if (e != hipSuccess) return hip_fail(e, "transcode_offsets_kernel");
    r.totals.assign((size_t)r.n_scans, 0);
    r.base.assign((size_t)r.n_scans, 0);
    if (r.n_scans) {
        e = hipMemcpyAsync(r.totals.data(), d_totals_.ptr, r.totals.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx_->stream);
        if (e != hipSuccess) return hip_fail(e, "hipMemcpyAsync(totals)");
    }
    r.sub_total_bits.assign((size_t)r.n_sub_scans, 0);
    if (r.n_sub_scans) {
        e = launch_subseq_transcode(ctx_->stream, 1, r.udata, r.scans, (const HuffWork *)d_sub_work_.ptr, r.n_sub_work, r.ends_u, r.status, r.pool, r.exit_state,
                                    r.first_block, nullptr, (const EncHuffTable *)d_enc_.ptr, (uint32_t *)d_sub_bits_.ptr, nullptr, nullptr, nullptr, r.n_slots);
        if (e != hipSuccess) return hip_fail(e, "subseq_transcode_kernel<measure>");
        e = launch_subseq_bit_offsets(ctx_->stream, r.scans, (const uint32_t *)d_sub_scan_ids_.ptr, r.n_sub_scans, (const uint32_t *)d_sub_bits_.ptr,
                                      (uint64_t *)d_sub_bitoff_.ptr, (uint64_t *)d_sub_totals_.ptr);
        if (e != hipSuccess) return hip_fail(e, "subseq_bit_offsets_kernel");
        e = hipMemcpyAsync(r.sub_total_bits.data(), d_sub_totals_.ptr, r.sub_total_bits.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx_->stream);
        if (e != hipSuccess) return hip_fail(e, "hipMemcpyAsync(bit totals)");
    }
    e = hipStreamSynchronize(ctx_->stream);
    if (e != hipSuccess) return hip_fail(e, "hipStreamSynchronize");
    uint64_t out_bytes = 0;
    for (int k = 0; k < r.n_scans; k++) {
        r.base[k] = out_bytes;
        out_bytes = (out_bytes + r.totals[k] + 255) & ~(uint64_t)255;
    }
    e = d_out_.reserve((size_t)out_bytes + 256);
    if (e != hipSuccess) return hip_fail(e, "hipMalloc(optimizer output)");
    return JPGPU_OK;
}

// ---- ... the scans with restart intervals: offsets, bytes
int OptimizeBatch::emit_intervals(Run &r) {
    hipError_t e;
    if (r.n_scans) {
        e = hipMemcpyAsync(d_base_.ptr, r.base.data(), r.base.size() * sizeof(uint64_t), hipMemcpyHostToDevice, ctx_->stream);
        if (e != hipSuccess) return hip_fail(e, "hipMemcpyAsync(bases)");
    }
    e = launch_transcode_offsets(ctx_->stream, r.scans, (const uint32_t *)d_scan_ids_.ptr, r.n_scans, (const uint32_t *)d_sizes_.ptr,
                                 (const uint64_t *)d_base_.ptr, (uint64_t *)d_offsets_.ptr, nullptr);
    if (e != hipSuccess) return hip_fail(e, "transcode_offsets_kernel");
    e = launch_transcode(ctx_->stream, 2, r.udata, r.input, r.scans, (const HuffWork *)d_work_.ptr, r.n_work, r.ends_u, r.ends_raw, r.status, r.pool, nullptr,
                         (const EncHuffTable *)d_enc_.ptr, (uint32_t *)d_sizes_.ptr, (const uint64_t *)d_offsets_.ptr, (uint8_t *)d_out_.ptr, r.n_slots);
    if (e != hipSuccess) return hip_fail(e, "transcode_kernel<emit>");
    return JPGPU_OK;
}

// ---- ... the DRI = 0 scans: raw (unstuffed) bit buffers + the encoder's stuffing stage (E4), descriptors in the encoder's image form
// (header_len, restart_interval and n_units zero: nothing in front of the stream, no restart marks)
int OptimizeBatch::emit_subsequences_and_stuff(Run &r) {
    r.simages.assign((size_t)r.n_sub_scans, DevEncImage());
    memset(r.simages.data(), 0, r.simages.size() * sizeof(DevEncImage));
    const StuffPlan sp = plan_stuffing_layout(r.simages.data(), r.sub_total_bits.data(), r.n_sub_scans, true);
    std::vector<uint64_t> scan_raw_off(r.n_jobs, 0);
    for (int k = 0; k < r.n_sub_scans; k++) scan_raw_off[sub_scan_ids_[k]] = r.simages[k].raw_off;
    const DevUpload grow[] = {{&d_raw_, nullptr, 0, (size_t)sp.raw_bytes + 256},
                              {&d_sout_, nullptr, 0, (size_t)sp.out_bytes + 256},
                              {&d_chunk_ff_, nullptr, 0, (size_t)sp.chunks * sizeof(uint32_t) + 256},
                              {&d_swork_chunk_, nullptr, 0, sp.work_chunk.size() * sizeof(EncWork) + 16}};
    bool copying = false;
    hipError_t e = reserve_and_copy(grow, ctx_->stream, &copying);
    if (e != hipSuccess) return hip_fail(e, "hipMalloc(optimizer raw buffers)");
    e = hipMemsetAsync(d_raw_.ptr, 0, (size_t)sp.raw_bytes + 256, ctx_->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_scan_raw_off_.ptr, scan_raw_off.data(), scan_raw_off.size() * sizeof(uint64_t), hipMemcpyHostToDevice, ctx_->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_simages_.ptr, r.simages.data(), r.simages.size() * sizeof(DevEncImage), hipMemcpyHostToDevice, ctx_->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_swork_chunk_.ptr, sp.work_chunk.data(), sp.work_chunk.size() * sizeof(EncWork), hipMemcpyHostToDevice, ctx_->stream);
    if (e != hipSuccess) return hip_fail(e, "hipMemcpyAsync(optimizer raw descriptors)");
    e = launch_subseq_transcode(ctx_->stream, 2, r.udata, r.scans, (const HuffWork *)d_sub_work_.ptr, r.n_sub_work, r.ends_u, r.status, r.pool, r.exit_state,
                                r.first_block, nullptr, (const EncHuffTable *)d_enc_.ptr, (uint32_t *)d_sub_bits_.ptr, (const uint64_t *)d_sub_bitoff_.ptr,
                                (const uint64_t *)d_scan_raw_off_.ptr, (uint8_t *)d_raw_.ptr, r.n_slots);
    if (e != hipSuccess) return hip_fail(e, "subseq_transcode_kernel<emit>");
    e = launch_stuff(ctx_->stream, (const DevEncImage *)d_simages_.ptr, (const EncWork *)d_swork_chunk_.ptr, (int)sp.work_chunk.size(),
                     (const uint64_t *)d_sub_totals_.ptr, (const uint8_t *)d_raw_.ptr, nullptr /* no restart marks: restart_interval is 0 */,
                     (uint32_t *)d_chunk_ff_.ptr, (uint8_t *)d_sout_.ptr, (uint64_t *)d_sout_len_.ptr);
    if (e != hipSuccess) return hip_fail(e, "stuff kernels");
    r.sout_len.assign((size_t)r.n_sub_scans, 0);
    e = hipMemcpyAsync(r.sout_len.data(), d_sout_len_.ptr, r.sout_len.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx_->stream);
    if (e != hipSuccess) return hip_fail(e, "hipMemcpyAsync(stuffed lengths)");
    return JPGPU_OK;
}

// where every file's scan data lies and how long the file is
void OptimizeBatch::collect_lengths(const Run &r) {
    int k = 0, ks = 0;
    for (Plan &p : plans_) {
        if (p.status != JPGPU_OK || p.job < 0) continue;
        if (p.transform.coefficient_road()) {  // a turned or cut image: the encoder's stuffing stage has closed its stream with EOI, too
            p.entropy_off = road_.images[(size_t)p.turn].out_off;
            p.entropy_len = road_.tail.h_out_len[(size_t)p.turn] >= 2 ? road_.tail.h_out_len[(size_t)p.turn] - 2 : 0;
        } else if (p.by_subsequence) {
            p.entropy_off = r.simages[ks].out_off;
            p.entropy_len = r.sout_len[ks] >= 2 ? r.sout_len[ks] - 2 : 0;  // the stuffing stage closes with EOI: that belongs to the host pieces here
            ks++;
        } else {
            p.entropy_off = r.base[k];
            p.entropy_len = r.totals[k];
            k++;
        }
        p.out_len = 0;
        for (const Piece &pc : p.pieces)
            p.out_len += pc.kind == Piece::kBytes ? pc.bytes.size() : (pc.kind == Piece::kHuffmanTables ? p.dht.size() : p.entropy_len);
    }
}

// ------------------------------------------------------------------------------------------------ lossless transform
// (include/jpgpu.h section (5), "Lossless transform")

int OptimizeBatch::set_orientation_policy(int policy) {
    if (policy != JPGPU_ORIENT_STORED && policy != JPGPU_ORIENT_FILE) return fail(JPGPU_ERR_ARGUMENT, "jpgpu_optimizer_set_orientation_policy: unknown policy");
    orient_policy_ = policy;
    return JPGPU_OK;
}
int OptimizeBatch::set_orientations(const uint8_t *orientations, int n) {
    if (n < 0 || (n > 0 && !orientations)) return fail(JPGPU_ERR_ARGUMENT, "jpgpu_optimizer_set_orientations: bad argument");
    for (int i = 0; i < n; i++)
        if (orientations[i] > 8) return fail(JPGPU_ERR_ARGUMENT, "jpgpu_optimizer_set_orientations: an orientation is 1..8, or 0 for what the policy gives");
    pending_orientations_.assign(orientations, orientations + n);
    return JPGPU_OK;
}
int OptimizeBatch::set_edge_policy(int edge) {
    if (edge != JPGPU_EDGE_REFUSE && edge != JPGPU_EDGE_TRIM) return fail(JPGPU_ERR_ARGUMENT, "jpgpu_optimizer_set_edge_policy: unknown policy");
    edge_policy_ = edge;
    return JPGPU_OK;
}
int OptimizeBatch::image_transform(int i, jpgpu_transform_info *info) const {
    if (i < 0 || i >= (int)plans_.size() || !info) return JPGPU_ERR_ARGUMENT;
    transform_info_of(plans_[(size_t)i].transform, info);
    return JPGPU_OK;
}
int OptimizeBatch::set_origin_policy(int origin) {
    if (origin != JPGPU_ORIGIN_REFUSE && origin != JPGPU_ORIGIN_EXPAND) return fail(JPGPU_ERR_ARGUMENT, "jpgpu_optimizer_set_origin_policy: unknown policy");
    origin_policy_ = origin;
    return JPGPU_OK;
}
int OptimizeBatch::set_windows(const jpgpu_rect *windows, int n) {
    if (n < 0 || (n > 0 && !windows)) return fail(JPGPU_ERR_ARGUMENT, "jpgpu_optimizer_set_windows: bad argument");
    pending_windows_.assign(windows, windows + n);
    return JPGPU_OK;
}
int OptimizeBatch::image_window(int i, jpgpu_rect *applied) const {
    if (i < 0 || i >= (int)plans_.size() || !applied) return JPGPU_ERR_ARGUMENT;
    const TransformPlan &tp = plans_[(size_t)i].transform;
    *applied = tp.has_window ? tp.applied : jpgpu_rect{0, 0, tp.out_width, tp.out_height};
    return JPGPU_OK;
}

// The host side of a turned image: its plan, and the pieces of Optimize(strip) over F' -- the source with the SOF, DQT and Exif patches.
// An image whose orientation is 1 is never touched: with nothing set (no list, the STORED policy) or a 1 in the list the file is not even
// looked at, and a file whose headers plan_transform cannot walk is not turned -- it keeps whatever the optimizer's own walks make of it.
// A window ("Window" of the same section) puts the image on this road whatever its orientation, and there an unwalkable file FAILS with the
// plan's header error: a caller who asked for a region must not get the whole picture back.  The pieces are then those of F''.
void OptimizeBatch::plan_turned_image(Plan &p, const uint8_t *data, size_t len, bool strip, int given, const jpgpu_rect *window) {
    TransformPlan &tp = p.transform;
    tp = TransformPlan();
    const bool windowed = window && (window->x | window->y | window->width | window->height) != 0;
    if (!windowed && (given == 1 || (given == 0 && orient_policy_ == JPGPU_ORIENT_STORED))) return;
    if (const int rc = plan_transform(data, len, given, orient_policy_, edge_policy_, &tp, windowed ? window : nullptr, origin_policy_); rc != JPGPU_OK) {
        if (windowed) refuse(rc, tp.message, kDetailBadHeader);
        tp = TransformPlan();
        return;
    }
    if (!tp.coefficient_road()) return;
    if (tp.status != JPGPU_OK) refuse(tp.status, tp.message, tp.status == JPGPU_ERR_ARGUMENT ? kDetailNone : kDetailUnsupportedFrame);
    std::string f((const char *)data, len);
    uint8_t *b = (uint8_t *)&f[0];
    patch_turned_file(b, len, tp);
    WalkPlan turned;
    ScanEndCache ends;  // (of `f`, which goes away here)
    walk_file(turned, ends, b, len, strip, false, true);
    p.pieces = std::move(turned.pieces);
}

// The turned images of an upload: the files once more, as the decoder takes them, and the plans of KX and of the encoder's entropy stages
int OptimizeBatch::plan_road(const Upload &u) {
    static_cast<RoadPlans &>(road_) = RoadPlans();
    if (u.turned.empty()) {  // nothing of an earlier upload's turned images stays on the device
        road_.release();
        return JPGPU_OK;
    }
    // entries that are the same file (the same pointer and length: one canvas cut into tiles) take ONE slot of the second batch and are
    // entropy-decoded once; their descriptors share its place in the dense store
    std::vector<const uint8_t *> files;
    std::vector<size_t> lens;
    std::vector<int> slot_of;  // per entry of u.turned
    std::map<std::pair<const uint8_t *, size_t>, int> slots;
    for (const int i : u.turned) {
        const auto at = slots.emplace(std::make_pair(u.jpeg[i], u.len[i]), (int)files.size());
        if (at.second) {
            files.push_back(u.jpeg[i]);
            lens.push_back(u.len[i]);
        }
        slot_of.push_back(at.first->second);
    }
    road_.sources = (int)files.size();
    if (!road_.batch) road_.batch.reset(new DeviceBatch(ctx_));
    const int rc = road_.batch->upload_files(files.data(), lens.data(), (int)files.size(), JPGPU_FMT_PLANAR_U8);
    if (rc != JPGPU_OK) return rc;
    for (size_t k = 0; k < u.turned.size(); k++) {
        Plan &p = plans_[(size_t)u.turned[k]];
        const ImagePlan *img = road_.batch->image(slot_of[k]);
        if (img->status != JPGPU_OK) {
            static_cast<Verdict &>(p) = {img->status, img->detail, img->error};
            p.pieces.clear();
        } else if (!plan_road_image(p, img)) {
            p.status = JPGPU_ERR_NOT_SUPPORTED;
            p.detail = kDetailUnsupportedFrame;
            p.pieces.clear();
        }
    }
    const size_t nt = road_.images.size(), nw = road_.work_blk.size(), slack = 16;
    const DevUpload ups[] = {
        {&road_.d_turn_images, road_.turn_images.data(), nt * sizeof(DevTurnImage), nt * sizeof(DevTurnImage) + slack},
        {&road_.d_turn_work, road_.turn_work.data(), road_.turn_work.size() * sizeof(TurnWork), road_.turn_work.size() * sizeof(TurnWork) + slack},
        {&road_.d_layouts, road_.layouts.data(), nt * sizeof(DevEncLayout), nt * sizeof(DevEncLayout) + slack},
        {&road_.d_work_blk, road_.work_blk.data(), nw * sizeof(EncWork), nw * sizeof(EncWork) + slack},
        {&road_.d_work_stat, road_.work_stat.data(), road_.work_stat.size() * sizeof(EncWork), road_.work_stat.size() * sizeof(EncWork) + slack},
        {&road_.d_images, nullptr, 0, nt * sizeof(DevEncImage) + 256 + slack},
        {&road_.d_coefs, nullptr, 0, (size_t)road_.blocks_total * 128 + 256 + slack},
        {&road_.d_hist, nullptr, 0, nt * 8 * 256 * sizeof(uint32_t) + 256 + slack},
        {&road_.d_tables, nullptr, 0, nt * 8 * sizeof(EncHuffTable) + 256 + slack},
    };
    bool copying = false;
    hipError_t e = reserve_and_copy(ups, ctx_->stream, &copying);
    if (e != hipSuccess) return hip_fail(e, copying ? "hipMemcpyAsync(lossless transform plans)" : "hipMalloc");
    if ((e = road_.tail.reserve(road_.blocks_total, nw, nt)) != hipSuccess) return hip_fail(e, road_.tail.failed);
    return JPGPU_OK;
}

// One image of the coefficient road: DevTurnImage (KX), DevEncImage and DevEncLayout (the encoder's general kernels) from its TransformPlan
// and the optimizer's view of its scan, whose table slots are the builders' order.  false: refused, the reason in p.error.
bool OptimizeBatch::plan_road_image(Plan &p, const ImagePlan *img) {
    const TransformPlan &tp = p.transform;
    const ScanJob &job = batch_.jobs_[p.job];
    uint32_t bpm = 0;
    for (int c = 0; c < tp.ncomp; c++) bpm += (uint32_t)tp.h[c] * tp.v[c];
    bool expressible = img->jobs.size() == 1 && road_.batch->jobs_[img->jobs[0]].kind == kScanSequential && job.scan_components == tp.ncomp &&
                       img->mcus_per_line == tp.src_mcus_per_line && img->mcus_per_column == tp.src_mcus_per_column && img->blocks_per_mcu == bpm &&
                       img->total_blocks == (uint64_t)tp.src_mcus_per_line * tp.src_mcus_per_column * bpm && job.n_huff <= 8;
    for (int c = 0; expressible && c < tp.ncomp; c++)
        expressible = job.comp[c].h == tp.h[c] && job.comp[c].v == tp.v[c] && job.dc_slot[c] < 8 && job.ac_slot[c] < 8;
    if (!expressible) {
        p.error = "The arrangement of this scan cannot be turned.";
        return false;
    }
    const bool tr = tp.transposes();
    DevTurnImage g;
    memset(&g, 0, sizeof g);
    DevEncImage im;
    memset(&im, 0, sizeof im);
    DevEncLayout L;
    memset(&L, 0, sizeof L);
    g.src_off = img->coef_offset;
    g.dst_off = road_.blocks_total;
    g.orientation = (uint32_t)tp.orientation;
    g.bpm = bpm;
    g.src_mcus_per_line = tp.src_mcus_per_line;
    g.kept_mcus_per_line = tp.kept_mcus_per_line;
    g.kept_mcus_per_column = tp.kept_mcus_per_column;
    g.dst_mcus_per_line = tr ? tp.kept_mcus_per_column : tp.kept_mcus_per_line;
    g.dst_mcus_per_column = tr ? tp.kept_mcus_per_line : tp.kept_mcus_per_column;
    if (tp.has_window) {  // the destination is the window's grid; plan_transform has checked that it lies inside the turned one
        if ((uint64_t)tp.win_mcu_x + tp.win_mcus_per_line > g.dst_mcus_per_line || (uint64_t)tp.win_mcu_y + tp.win_mcus_per_column > g.dst_mcus_per_column) {
            p.error = "The window does not lie inside the MCU grid of the turned image.";
            return false;
        }
        g.origin_mx = tp.win_mcu_x;
        g.origin_my = tp.win_mcu_y;
        g.dst_mcus_per_line = tp.win_mcus_per_line;
        g.dst_mcus_per_column = tp.win_mcus_per_column;
    }
    g.total_blocks = g.dst_mcus_per_line * g.dst_mcus_per_column * bpm;
    L.ncomp = (uint32_t)tp.ncomp;
    L.max_h = tr ? tp.max_v : tp.max_h;
    L.max_v = tr ? tp.max_h : tp.max_v;
    L.own_blocks = 1;  // (statistics are taken; the grids below are the whole MCU grid, so no block is the allocator's dummy)
    L.table_base = (uint32_t)(8 * road_.images.size());
    L.hist_index = (uint32_t)(8 * 256 * road_.images.size());
    uint32_t b = 0;
    for (int c = 0; c < tp.ncomp; c++) {
        const uint32_t h = tr ? tp.v[c] : tp.h[c], v = tr ? tp.h[c] : tp.v[c];
        g.src_h[c] = tp.h[c];
        g.src_v[c] = tp.v[c];
        g.first_blk[c] = (uint8_t)b;
        L.h[c] = (uint8_t)h;
        L.v[c] = (uint8_t)v;
        L.hs[c] = (uint8_t)(L.max_h / h);
        L.vs[c] = (uint8_t)(L.max_v / v);
        L.dc_slot[c] = job.dc_slot[c];
        L.ac_slot[c] = job.ac_slot[c];
        L.first_blk[c] = (uint8_t)b;
        L.grid_w[c] = g.dst_mcus_per_line * h;
        L.grid_h[c] = g.dst_mcus_per_column * v;
        for (uint32_t y = 0; y < v; y++)
            for (uint32_t x = 0; x < h; x++) {
                g.blk[b] = (uint8_t)((uint32_t)c | x << 2 | y << 4);
                L.blk_comp[b] = (uint8_t)c;
                L.blk_x[b] = (uint8_t)x;
                L.blk_y[b] = (uint8_t)y;
                L.blk_info[b] = (uint32_t)c | (x << 2) | (y << 4) | (h << 6) | (v << 9) | ((uint32_t)job.dc_slot[c] << 12) | ((uint32_t)job.ac_slot[c] << 15) |
                                ((uint32_t)L.first_blk[c] << 18) | (((uint32_t)L.first_blk[c] + h * v - 1u) << 24);
                b++;
            }
    }
    im.coef_off = g.dst_off;
    im.width = tp.out_width;
    im.height = tp.out_height;
    im.components = (uint32_t)tp.ncomp;
    im.luma_h = L.max_h;
    im.luma_v = L.max_v;
    im.mcus_per_line = g.dst_mcus_per_line;
    im.mcus_per_column = g.dst_mcus_per_column;
    im.bpm = bpm;
    im.total_blocks = g.total_blocks;
    im.restart_interval = (uint32_t)p.dri_at_scan;
    const uint32_t mcus = im.mcus_per_line * im.mcus_per_column;
    im.n_units = im.restart_interval ? (mcus + im.restart_interval - 1) / im.restart_interval : im.total_blocks;
    im.work_first = (uint32_t)road_.work_blk.size();
    im.layout = (uint32_t)road_.layouts.size() + 1;
    p.turn = (int)road_.images.size();
    for (uint32_t f = 0; f < g.total_blocks; f += kTurnBlocksPerWg) road_.turn_work.push_back({(uint32_t)p.turn, f});
    for (uint32_t f = 0; f < im.n_units; f += 256) road_.work_blk.push_back({(uint32_t)p.turn, f});
    for (uint32_t f = 0; f < im.total_blocks; f += 256) road_.work_stat.push_back({(uint32_t)p.turn, f});
    road_.blocks_total += g.total_blocks;
    road_.turn_images.push_back(g);
    road_.images.push_back(im);
    road_.layouts.push_back(L);
    return true;
}

// ---- the turned images: K1 + K2 of the decoder fill its coefficient store; KX reads it dense
int OptimizeBatch::decode_turned(Run &r) {
    (void)hipEventRecord(road_.ev_td[0], ctx_->stream);
    road_.batch->note_entropy_only_request();
    int rc = road_.batch->run_marker_index();
    if (rc == JPGPU_OK) rc = road_.batch->run_huffman();
    (void)hipEventRecord(road_.ev_td[1], ctx_->stream);
    // (what a reader of the store owes the batch, as jpgpu_batch_download_coefficients pays it: DRI = 0 scans are decoded in rounds whose
    // count the host confirms here, issuing the stage again where they did not suffice)
    if (rc == JPGPU_OK) rc = road_.batch->sync();
    if (rc != JPGPU_OK) return rc;
    r.turn_src = (const int16_t *)road_.batch->coefs_device(nullptr);  // (expands the scans K2 handed over as half-line planes)
    (void)hipEventRecord(road_.ev_td[2], ctx_->stream);
    if (!r.turn_src) return fail(JPGPU_ERR_DEVICE, "the dense coefficient store of the turned images is not available");
    return JPGPU_OK;
}

// ---- KX: every block to its place in the turned grid, sign-flipped and transposed (kx_lossless.hip)
int OptimizeBatch::turn_blocks(Run &r) {
    (void)hipEventRecord(road_.ev_kx[0], ctx_->stream);
    hipError_t e = launch_lossless_turn(ctx_->stream, (const DevTurnImage *)road_.d_turn_images.ptr, (const TurnWork *)road_.d_turn_work.ptr, (int)road_.turn_work.size(), r.turn_src,
                                        (int16_t *)road_.d_coefs.ptr);
    (void)hipEventRecord(road_.ev_kx[1], ctx_->stream);
    if (e != hipSuccess) return hip_fail(e, "lossless_turn_kernel");
    return JPGPU_OK;
}

// ---- statistics of the turned blocks (the encoder's GatherBlockStatistics) and Build per (class, identifier) of the source's DHT
int OptimizeBatch::build_turned_tables(Run &r) {
    const size_t n_hist = (size_t)r.n_turned * 8 * 256;
    hipError_t e = hipMemcpyAsync(road_.d_images.ptr, road_.images.data(), road_.images.size() * sizeof(DevEncImage), hipMemcpyHostToDevice, ctx_->stream);
    if (e == hipSuccess) e = hipMemsetAsync(road_.d_hist.ptr, 0, n_hist * sizeof(uint32_t), ctx_->stream);
    if (e != hipSuccess) return hip_fail(e, "hipMemsetAsync(turned statistics)");
    e = launch_block_stats(ctx_->stream, (const DevEncImage *)road_.d_images.ptr, (const EncWork *)road_.d_work_stat.ptr, (int)road_.work_stat.size(),
                           (const int16_t *)road_.d_coefs.ptr, (uint32_t *)road_.d_hist.ptr, (const DevEncLayout *)road_.d_layouts.ptr, false);
    if (e != hipSuccess) return hip_fail(e, "block_stats_kernel");
    std::vector<uint32_t> hist(n_hist);
    e = hipMemcpyAsync(hist.data(), road_.d_hist.ptr, hist.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx_->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx_->stream);
    if (e != hipSuccess) return hip_fail(e, "hipMemcpy(turned statistics)");
    std::vector<EncHuffTable> enc(8 * (size_t)r.n_turned);
    memset(enc.data(), 0, enc.size() * sizeof(EncHuffTable));
    for (Plan &p : plans_)  // (as build_tables reports it for the source's own statistics)
        if (p.turn >= 0) build_image_tables(p, &hist[(size_t)p.turn * 8 * 256], &enc[(size_t)p.turn * 8]);
    e = hipMemcpyAsync(road_.d_tables.ptr, enc.data(), enc.size() * sizeof(EncHuffTable), hipMemcpyHostToDevice, ctx_->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx_->stream);  // (`enc` leaves scope)
    if (e != hipSuccess) return hip_fail(e, "hipMemcpyAsync(turned encoding tables)");
    return JPGPU_OK;
}

// ---- bits, emit and stuffing through the encoder's general kernels (E2, E3, E4); no header in front of the streams
int OptimizeBatch::emit_turned(Run &r) {
    EntropyTail &t = road_.tail;
    const EntropyTail::Source src = {(const DevEncImage *)road_.d_images.ptr, (const EncWork *)road_.d_work_blk.ptr, (int)road_.work_blk.size(),
                                     (const EncHuffTable *)road_.d_tables.ptr, (const int16_t *)road_.d_coefs.ptr, (const DevEncLayout *)road_.d_layouts.ptr, false};
    hipError_t e = t.count_bits(ctx_->stream, src, r.n_turned);
    if (e == hipSuccess) e = t.read_bit_counts(ctx_->stream, r.n_turned);
    if (e == hipSuccess) e = t.plan(ctx_->stream, road_.images.data(), r.n_turned, true);
    if (e != hipSuccess) return hip_fail(e, t.failed);
    e = hipMemcpyAsync(road_.d_images.ptr, road_.images.data(), (size_t)r.n_turned * sizeof(DevEncImage), hipMemcpyHostToDevice, ctx_->stream);
    if (e != hipSuccess) return hip_fail(e, "hipMemcpyAsync(turned stream descriptors)");
    e = t.upload_chunk_work(ctx_->stream);
    if (e == hipSuccess) e = t.emit(ctx_->stream, src);
    if (e == hipSuccess) e = t.stuff_bytes(ctx_->stream, src.images);
    if (e == hipSuccess) e = t.read_lengths(ctx_->stream, r.n_turned);
    return e == hipSuccess ? JPGPU_OK : hip_fail(e, t.failed);
}

int OptimizeBatch::result(int i, jpgpu_image_result *res, size_t *out_len) {
    if (i < 0 || i >= (int)plans_.size() || !res) return fail(JPGPU_ERR_ARGUMENT, "jpgpu_optimizer_result: bad index");
    memset(res, 0, sizeof *res);
    if (out_len) *out_len = 0;
    const Plan &p = plans_[i];
    const auto report = [&](const Verdict &v) {
        res->status = v.status;
        res->detail = v.detail;
        ctx_->last_error = v.error;
    };
    if (p.status != JPGPU_OK) {
        report(p);
        return JPGPU_OK;
    }
    if (!ran_) return fail(JPGPU_ERR_INVALID_OPERATION, "jpgpu_optimizer_result: run() has not completed");
    int rc = batch_.result(i, res);  // device-side scan errors, with the reference's exception classes
    if (rc != JPGPU_OK) return rc;
    if (res->status == JPGPU_OK) {
        // a restart check that meets EOI (early EOI, or an MCU count that is a multiple of DRI) makes Scan() return before
        // it builds its tables (:437-442); Optimize() then throws InvalidOperationException (:542-545)
        const DevScan &s = batch_.h_scans_[p.job];
        const DevScanStatus &st = batch_.h_status_[p.job];
        // (a windowed image: the restart rule is that of F'', checked below -- the MCU count of the source does not decide it)
        const bool count_decides = s.restart_check_at_end != 0 && !p.transform.has_window;
        const bool check_saw_eoi = s.dri != 0 && st.terminator == 0xD9 && (st.n_ends < s.n_intervals || (st.n_ends == s.n_intervals && count_decides));
        if (check_saw_eoi) {
            res->status = JPGPU_ERR_INVALID_OPERATION;
            ctx_->last_error = "Operation is not valid due to the current state of the object.";
        } else if (st.terminator == 0 && st.pad[2] >= 8) {
            // the data ran out behind the scan with whole bytes left and no marker among them: Scan()'s marker loop fails (:82-86)
            res->status = JPGPU_ERR_INVALID_DATA;
            res->detail = kDetailBadHeader;
            ctx_->last_error = "Failed to decode JPEG data at offset " + std::to_string(batch_.image(i)->file_len) + ". No marker found.";
        } else if (st.terminator != 0 && (st.terminator & 0xF8u) != 0xD0u && (st.pad[2] >> 3) == 1) {
            report(p.swallow);
        } else if (p.late.status != JPGPU_OK) {
            report(p.late);
        }
    }
    if (res->status == JPGPU_OK && p.turn >= 0) {
        // the same restart check on F': a trimmed image has fewer MCUs than its source, and where their count is a multiple of DRI Scan() of
        // F' returns before it builds its tables, as above
        const DevEncImage &im = road_.images[(size_t)p.turn];
        if (im.restart_interval != 0 && (im.mcus_per_line * im.mcus_per_column) % im.restart_interval == 0) {
            res->status = JPGPU_ERR_INVALID_OPERATION;
            ctx_->last_error = "Operation is not valid due to the current state of the object.";
        }
    }
    if (res->status == JPGPU_OK && out_len) *out_len = (size_t)p.out_len;
    return JPGPU_OK;
}

int OptimizeBatch::download(int i, void *dst, size_t cap) {
    jpgpu_image_result res;
    size_t n = 0;
    int rc = result(i, &res, &n);
    if (rc != JPGPU_OK) return rc;
    if (res.status != JPGPU_OK) return fail(res.status, ctx_->last_error);
    if (!dst || cap < n) return fail(JPGPU_ERR_ARGUMENT, "jpgpu_optimizer_download: buffer too small");
    const Plan &p = plans_[i];
    uint8_t *o = (uint8_t *)dst;
    for (const Piece &pc : p.pieces) {
        if (pc.kind == Piece::kBytes) {
            memcpy(o, pc.bytes.data(), pc.bytes.size());
            o += pc.bytes.size();
        } else if (pc.kind == Piece::kHuffmanTables) {
            memcpy(o, p.dht.data(), p.dht.size());
            o += p.dht.size();
        } else if (p.entropy_len) {
            const uint8_t *src = (const uint8_t *)(p.turn >= 0 ? road_.tail.out.ptr : (p.by_subsequence ? d_sout_.ptr : d_out_.ptr)) + p.entropy_off;
            hipError_t e = hipMemcpy(o, src, (size_t)p.entropy_len, hipMemcpyDeviceToHost);
            if (e != hipSuccess) return hip_fail(e, "hipMemcpy(optimizer output)");
            o += p.entropy_len;
        }
    }
    return JPGPU_OK;
}

bool OptimizeBatch::statistics(int i, int t, uint8_t *table_class, uint8_t *identifier, uint32_t counts[256]) const {
    if (i < 0 || i >= (int)plans_.size() || !ran_) return false;
    const Plan &p = plans_[i];
    if (p.status != JPGPU_OK || p.job < 0) return false;
    const ScanJob &job = batch_.jobs_[p.job];
    if (t < 0 || t >= job.n_huff) return false;
    *table_class = job.huff_copy[t].table_class;
    *identifier = job.huff_copy[t].identifier;
    memcpy(counts, &h_hist_[((size_t)p.job * kMaxHuffSlots + t) * 256], 256 * sizeof(uint32_t));
    return true;
}

}  // namespace jpgpu
