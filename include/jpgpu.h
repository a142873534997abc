/*
 * include/jpgpu.h -- C ABI of the MI355X-native baseline-JPEG decode path (libjpgpu.so).
 *
 * This is the drop-in boundary for yigolden/JpegLibrary's hot path
 *     JpegDecoder.Decode() -> JpegHuffmanBaselineScanDecoder.ProcessScan -> JpegBlockOutputWriter.WriteBlock
 * Every entry point names the reference interface it replaces ("ref:", paths relative to
 * /root/reference/src/JpegLibrary).  Plain pointers and sizes only; no C++/torch types.
 * INTEGRATION.md shows the C# P/Invoke stubs that bind these symbols.
 *
 * Three levels:
 *   (1) jpgpu_batch_*    whole-file batch decode with device-resident inputs/outputs (throughput path, bench)
 *   (2) jpgpu_decode_scan  one scan with pre-parsed tables (what a C# JpegScanDecoder replacement P/Invokes)
 *   (3) jpgpu_decoder_*  handle-based mirror of the public JpegDecoder API (Identify / SetOutputWriter / Decode)
 *
 * Threading: a ctx owns one device + one HIP stream; calls on one ctx (and objects made from it) must be
 * serialised by the caller; different ctxs are independent (one per GPU / per thread).
 */
#ifndef JPGPU_H
#define JPGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 101: jpgpu_image_result gained error_block (28 bytes, 24 before) and the library writes all of it: a binding compiled against
 * an older header must refuse to run -- compare jpgpu_version() / jpgpu_sizeof_image_result() with its own at load time. */
#define JPGPU_VERSION 101

/* ---- status codes.  1..4 mirror the reference's exception classes so a shim can rethrow them. ---- */
typedef enum jpgpu_status {
    JPGPU_OK = 0,
    JPGPU_ERR_INVALID_DATA = 1,      /* System.IO.InvalidDataException   (ref: ScanDecoder/JpegScanDecoder.cs:39-48) */
    JPGPU_ERR_INVALID_OPERATION = 2, /* System.InvalidOperationException (ref: JpegDecoder.cs:513-518)               */
    JPGPU_ERR_NOT_SUPPORTED = 3,     /* System.NotSupportedException     (ref: JpegDecoder.cs:629)                   */
    JPGPU_ERR_ARGUMENT = 4,          /* System.ArgumentException family                                              */
    JPGPU_ERR_DEVICE = 5,            /* HIP runtime failure (message in jpgpu_last_error)                            */
    JPGPU_ERR_NO_DEVICE = 6,         /* no MI355X visible: the product has NO CPU fallback                           */
    JPGPU_ERR_OUT_OF_MEMORY = 7
} jpgpu_status;

/* Per-image detail codes reported by the device kernels (jpgpu_image_result.detail). */
typedef enum jpgpu_detail {
    JPGPU_DETAIL_NONE = 0,
    JPGPU_DETAIL_INVALID_HUFFMAN_CODE = 1, /* "Invalid Huffman code encountered."  ref: JpegHuffmanDecodingTable.cs:104 */
    JPGPU_DETAIL_MARKER_IN_DATA = 2,       /* "Expect raw data from bit stream. Yet a marker is encountered." ref: ScanDecoder/JpegHuffmanScanDecoder.cs:107 */
    JPGPU_DETAIL_STREAM_ENDED = 3,         /* "The bit stream ended prematurely."  ref: ScanDecoder/JpegHuffmanScanDecoder.cs:109 */
    JPGPU_DETAIL_EXPECT_RESTART = 4,       /* "Expect restart marker."  ref: ScanDecoder/JpegHuffmanBaselineScanDecoder.cs:153 */
    JPGPU_DETAIL_MISSING_TABLE = 5,        /* Huffman / quantization table not defined. ref: ...BaselineScanDecoder.cs:72-81 */
    JPGPU_DETAIL_UNSUPPORTED_FRAME = 6,    /* SOF other than SOF0/SOF1 on this path */
    JPGPU_DETAIL_BAD_HEADER = 7,           /* marker/segment parse failure before the scan */
    JPGPU_DETAIL_EARLY_EOI = 8,            /* not an error: EOI met at a restart boundary, image partially decoded (ref: ...BaselineScanDecoder.cs:145-150) */
    JPGPU_DETAIL_UNEXPECTED_END = 9,       /* "Unexpected end of JPEG data stream."  ref: ScanDecoder/JpegHuffmanProgressiveScanDecoder.cs:249,295,336,350,366,404 */
    JPGPU_DETAIL_NULL_TABLE = 10           /* optimizer: a block needs a Huffman table that was never defined (the reference dereferences null, JpegOptimizer.cs:468-480) */
} jpgpu_detail;

/* Output layouts. */
typedef enum jpgpu_format {
    /* "O2": interleaved u8, out[(y*W+x)*C + c], signed clamp to [0,255], sub-sampled components replicated,
     * clipped to W x H.  Byte-identical to apps/JpegDecode/JpegBufferOutputWriter8Bit.cs:28-60 with C = components. */
    JPGPU_FMT_INTERLEAVED_U8 = 0,
    /* planar u8 at component-native resolution, planes padded to whole MCUs, signed clamp to [0,255] */
    JPGPU_FMT_PLANAR_U8 = 1,
    /* "O1": planar int16 at component-native resolution, planes padded to whole MCUs, UNCLAMPED level-shifted
     * samples == the blocks JpegBlockOutputWriter.WriteBlock receives before chroma expansion
     * (ref: ScanDecoder/JpegHuffmanBaselineScanDecoder.cs:131-134) */
    JPGPU_FMT_PLANAR_I16 = 2,
    /* interleaved 8-bit R,G,B and R,G,B,A (A = 255): the step every caller of the reference runs right after the
     * decode, fused into the writer -- JpegYCbCrToRgbConverter.ConvertYCbCr8ToRgb24 / ConvertYCbCr8ToRgba32
     * (ref: apps/JpegDecode/JpegYCbCrToRgbConverter.cs:134-206, tables :66-118) applied to the "O2" samples; callers:
     * apps/JpegDecode/DecodeAction.cs:71-74, tests/JpegLibrary.Benchmarks/DecoderBenchmark.cs:67.  3-component frames;
     * 1-component frames are converted with Cb = Cr = 128 like DecodeAction.cs:57-65 does.  8-bit precision only. */
    JPGPU_FMT_RGB_U8 = 3,
    JPGPU_FMT_RGBA_U8 = 4,
    /* "O3": the sink of the reference's own decode tests, tests/JpegLibrary.Tests/Utils/JpegExtendingOutputWriter.cs:30-112
     * constructed with componentCount = 4 as HuffmanSequentialDecodeTests.cs:23-43 does: uint16 out[(y*W+x)*4 + c],
     * (ushort)sample clamped to 2^P - 1 (a negative sample becomes the maximum), the P bits spread over 16
     * (FastExpandBits / ExpandBits :86-111), sub-sampled components replicated like WriteBlockSlow, clipped to W x H;
     * channels >= the frame's component count stay zero.  What the golden PNG pairs of the reference hold. */
    JPGPU_FMT_EXTENDED_U16 = 5,
    /* INTERLEAVED_U8's geometry with the sample-to-byte step chosen by the frame's precision P the way
     * apps/JpegDecode/DecodeAction.cs:41-54 chooses its writer: P == 8 the bytes of INTERLEAVED_U8; 9 <= P <= 16
     * (byte)Clamp(sample >> (P - 8), 0, 255), an arithmetic shift (JpegBufferOutputWriterGreaterThan8Bit.cs:57,64-67);
     * 1 <= P <= 7 Clamp(sample, 0, 2^P - 1) (signed) spread over 8 bits by ExpandBits
     * (JpegBufferOutputWriterLessThan8Bit.cs:59-60, 67-93).  Any other P: the image fails by itself with
     * JPGPU_ERR_NOT_SUPPORTED / JPGPU_DETAIL_UNSUPPORTED_FRAME. */
    JPGPU_FMT_INTERLEAVED_U8_SCALED = 6,
    /* RGB_U8's bytes as three tight planes R, G, B of W x H each (pitch = W, no MCU padding): plane c at
     * out_offset + c * W * H, out_bytes = 3 * W * H -- the uint8[3, H, W] layout tensor code consumes, written by K3 itself.
     * The same conversion (ConvertYCbCr8ToRgb24 applied to the "O2" samples; 1-component frames with Cb = Cr = 128 give three
     * equal planes) and the same refusals as RGB_U8.  jpgpu_image_info.plane[0..2] describe the planes. */
    JPGPU_FMT_RGB_PLANAR_U8 = 7,
    /* RGB_PLANAR_U8's planes with a wider sample T = IEEE binary16 / binary32 -- the float16 / float32 [3, H, W] tensor a model or a float
     * resize starts from, written by K3 itself: plane c at out_offset + c * W * H * sizeof(T), out_bytes = 3 * W * H * sizeof(T);
     * jpgpu_image_info.plane[c] = {c * W * H * sizeof(T) (bytes), W, H, W (samples)}.  Sample (c, y, x), with u the byte RGB_PLANAR_U8
     * holds there and the constants of jpgpu_batch_set_output_affine (default: scale 1, bias 0):
     *     t = (float)u * scale[c]     one float32 multiply, rounded to nearest even
     *     v = t + bias[c]             one float32 add, rounded to nearest even; never fused with the multiply
     *     F32: v      F16: v rounded to nearest even to binary16 (subnormals kept, overflow to infinity)
     * i.e. numpy's (u.astype(float32) * float32(scale[c]) + float32(bias[c])).astype(float16).  The same refusals as RGB_U8, per image.  No
     * bfloat16, no interleaved (HWC) float form. */
    JPGPU_FMT_RGB_PLANAR_F16 = 8,
    JPGPU_FMT_RGB_PLANAR_F32 = 9
} jpgpu_format;

typedef struct jpgpu_ctx jpgpu_ctx;
typedef struct jpgpu_batch jpgpu_batch;
typedef struct jpgpu_decoder jpgpu_decoder;

/* ------------------------------------------------------------------------------------------------ context */

int jpgpu_version(void);
/* sizeof(jpgpu_image_result) as THIS library writes it (the struct every *_result call fills in whole). */
size_t jpgpu_sizeof_image_result(void);
/* Number of visible HIP devices (0 when none; never initialises a context). */
int jpgpu_device_count(void);
/* Creates a context on `device`.  Fails with JPGPU_ERR_NO_DEVICE when no GPU is present. */
int jpgpu_create(int device, jpgpu_ctx **out);
void jpgpu_destroy(jpgpu_ctx *ctx);
/* Last error text of this context (thread-compatible, not thread-safe). ctx may be NULL for create failures. */
const char *jpgpu_last_error(const jpgpu_ctx *ctx);
/* Host threads jpgpu_batch_upload may use for this context (header parsing of the files, copies into the pinned staging
 * ring, full marker walks of the files that need one).  0 = default: min(CPUs granted to the process, 16), or JPGPU_HOST_THREADS.
 * The reference is single-threaded per decoder ("one decoder per thread"); a batch is where the host fans out. */
int jpgpu_set_host_threads(jpgpu_ctx *ctx, int threads);
/* Page-locked host memory for the zero-copy ingest (jpgpu_batch_upload_segments with JPGPU_UPLOAD_PINNED).  The reference's
 * callers own their input (SetInput takes a ReadOnlyMemory / ReadOnlySequence<byte>, JpegDecoder.cs:49-62, filled e.g. by
 * apps/JpegDecode/MemoryPoolBufferWriter.cs); a C# shim either reads its files into jpgpu_host_alloc'd memory or pins its
 * own array (GCHandle) and registers it, so that the DMA engine reads the bytes where they lie.  Registration costs a few
 * microseconds per page: do it once per buffer, not per decode. */
int jpgpu_host_alloc(jpgpu_ctx *ctx, size_t bytes, void **out);
int jpgpu_host_free(jpgpu_ctx *ctx, void *p);
int jpgpu_host_register(jpgpu_ctx *ctx, void *p, size_t bytes);
int jpgpu_host_unregister(jpgpu_ctx *ctx, void *p);
/* Image-per-GPU sharding: of n_items, rank `rank` of `world` takes items first, first + stride, ... (count of
 * them): image i -> GPU i mod G.  Independent contexts, no exchange between them; any out pointer may be NULL. */
void jpgpu_shard(int n_items, int rank, int world, int *first, int *stride, int *count);
const char *jpgpu_status_string(int status);
const char *jpgpu_detail_string(int detail);

/* ------------------------------------------------------------------------------------------------ headers */

/* ref: JpegFrameHeader.cs (SOF payload) */
typedef struct jpgpu_frame_component {
    uint8_t identifier, h, v, tq;
} jpgpu_frame_component;
typedef struct jpgpu_frame {
    uint16_t width, height; /* SamplesPerLine, NumberOfLines */
    uint8_t precision, num_components;
    uint8_t sof; /* marker byte: 0xC0 / 0xC1 */
    uint8_t reserved;
    jpgpu_frame_component comp[4];
} jpgpu_frame;

/* ref: JpegScanHeader.cs (SOS payload) */
typedef struct jpgpu_scan_component {
    uint8_t selector, td, ta, reserved;
} jpgpu_scan_component;
typedef struct jpgpu_scan {
    uint8_t num_components, ss, se, ah, al;
    uint8_t reserved[3];
    jpgpu_scan_component comp[4];
} jpgpu_scan;

/* ref: JpegHuffmanDecodingTable.TryParse input: BITS[16] + HUFFVAL (DHT payload without the Tc/Th byte) */
typedef struct jpgpu_dht {
    uint8_t present;
    uint8_t bits[16];
    uint8_t num_values_minus_0; /* unused, kept for alignment */
    uint16_t num_values;
    uint8_t values[256];
} jpgpu_dht;

/* Geometry of one decoded image inside a batch's output buffer. */
typedef struct jpgpu_plane_info {
    uint64_t offset; /* bytes from the image's out_offset */
    uint32_t width, height, pitch; /* samples; pitch in samples */
} jpgpu_plane_info;
typedef struct jpgpu_image_info {
    int32_t status; /* host-side parse status (jpgpu_status) */
    int32_t detail;
    uint16_t width, height;
    uint8_t precision, num_components, sof, reserved;
    uint32_t restart_interval;
    uint32_t mcus_per_line, mcus_per_column, blocks_per_mcu;
    uint64_t total_blocks;
    uint64_t out_offset, out_bytes;   /* in the batch output buffer */
    uint64_t coef_offset;             /* first block index in the batch coefficient buffer */
    jpgpu_plane_info plane[4];        /* planar formats only (PLANAR_U8, PLANAR_I16, RGB_PLANAR_U8 / _F16 / _F32) */
} jpgpu_image_info;

typedef struct jpgpu_image_result {
    int32_t status; /* jpgpu_status */
    int32_t detail; /* jpgpu_detail */
    uint32_t error_interval;  /* restart interval index of the first failure */
    uint32_t decoded_mcus;    /* MCUs actually decoded (== total unless EARLY_EOI) */
    uint32_t bytes_consumed;  /* entropy bytes up to the terminating marker; same meaning as the reader advance in
                                 ref: ScanDecoder/JpegHuffmanBaselineScanDecoder.cs:167-176 for well-formed streams */
    uint32_t terminator;      /* marker byte that ended the entropy segment (0xD9 = EOI), 0 if the data ran out */
    uint32_t error_block;     /* a sequential scan that failed: index, in scan order, of the block the reference threw in -- it has
                                 called WriteBlock for every block in front of it and for none behind it
                                 (JpegHuffmanBaselineScanDecoder.cs:99-134, 153); 0xFFFFFFFF otherwise */
} jpgpu_image_result;

/* ------------------------------------------------------------------------------------------------ (1) batch
 * Replaces, for a whole set of files at once, the canonical call sequence of every reference caller
 *   new JpegDecoder(); SetInput; Identify; SetOutputWriter(JpegBufferOutputWriter8Bit); Decode()
 * (ref: apps/JpegDecode/DecodeAction.cs:26-56, tests/JpegLibrary.Benchmarks/DecoderBenchmark.cs:51-73).
 */
int jpgpu_batch_create(jpgpu_ctx *ctx, jpgpu_batch **out);
void jpgpu_batch_destroy(jpgpu_batch *b);

/* Host side of SetInput+Identify+the marker loop of Decode up to SOS (ref: JpegDecoder.cs:75-162, 509-617):
 * parses every file's headers/tables, builds device descriptors and uploads the compressed bytes to HBM.
 * `format` is a jpgpu_format.  Images whose headers fail to parse get a per-image status and are skipped.
 * Returns JPGPU_OK if the batch is usable (even if some images failed).  n == 0 (the arrays may be NULL) is an upload like any other: it
 * replaces what the batch held, jpgpu_batch_size is 0, jpgpu_batch_output_device reports no bytes, jpgpu_batch_decode and the stage calls
 * return JPGPU_OK without work, and every per-image call is refused for its index. */
int jpgpu_batch_upload(jpgpu_batch *b, const uint8_t *const *jpeg, const size_t *len, int n, int format);
/* The same for input that is not one contiguous span per file: file i consists of the next segments_per_file[i] entries of
 * `segments`, in order -- the ReadOnlySequence<byte> of JpegDecoder.SetInput (JpegDecoder.cs:56-62), which the reference reads
 * in place segment by segment (apps/JpegDecode/MemoryPoolBufferWriter.cs:166-174 builds such a sequence,
 * apps/JpegDecode/DecodeAction.cs:81-98 hands it over).  The host looks at the headers only (the first 64 KiB of a
 * multi-segment file are gathered for that; a file whose first scan starts later, or that needs the full marker walks, is
 * linearised on the host as a whole); the entropy-coded bytes travel segment by segment.
 * flags: JPGPU_UPLOAD_PINNED = every segment lies in page-locked memory (jpgpu_host_alloc / jpgpu_host_register): the
 * segments are DMA'd to HBM from where they lie -- no staging copy, no host thread touches the entropy bytes.  Without the
 * flag the segments go through the pinned staging ring like jpgpu_batch_upload's files.
 * Ordering: an upload is ordered behind device work this batch has issued and not yet synchronised (it will not overwrite
 * inputs a running decode of the SAME batch still reads); results of that earlier work are lost with the upload. */
typedef struct jpgpu_segment {
    const uint8_t *data;
    size_t len;
} jpgpu_segment;
#define JPGPU_UPLOAD_PINNED 1u
/* All segments lie inside ONE page-locked allocation (a read buffer the caller fills file after file), every file contiguous,
 * and the bytes BETWEEN the files belong to that allocation too (they are read, never interpreted): the device copy mirrors
 * the arena's layout and the whole span travels as a few large DMAs instead of one per file.  Falls back to one DMA per segment
 * when the files are not contiguous or the span is mostly gaps (more than twice the payload). */
#define JPGPU_UPLOAD_PINNED_ARENA 2u
int jpgpu_batch_upload_segments(jpgpu_batch *b, const jpgpu_segment *segments, const int *segments_per_file, int n, int format,
                                unsigned flags);
/* What the last jpgpu_batch_upload did.  The host reads headers only: both marker loops stop behind the first SOS header and
 * the file is planned as one sequential scan closed by EOI; the bytes behind the header are looked at by the device, which
 * reports the first marker that is not RSTn (what Identify's walk, JpegDecoder.cs:75-162 / JpegReader.cs:120-158, would
 * meet next).  n_header_only = files whose plan was confirmed that way; n_full_walk = files that took the full host walks
 * of Identify and Decode (several scans, progressive, segments or garbage behind the scan, truncated data).  The bytes
 * travel through a pinned staging ring on the context's upload stream, beside whatever runs on its decode stream. */
typedef struct jpgpu_ingest_stats {
    int32_t threads;        /* host threads used */
    int32_t n_header_only;
    int32_t n_full_walk;
    float parse_ms;         /* header-only plans */
    float copy_ms;          /* staging copies + H2D + device verdict */
    float full_walk_ms;     /* full marker walks (+ the reader-position verdicts of the confirmed plans) */
    float layout_ms;        /* descriptors, work lists, device allocations */
    float total_ms;
    int32_t n_pinned_dma;   /* segments sent by DMA straight from the caller's page-locked memory (JPGPU_UPLOAD_PINNED) */
    int32_t n_linearised;   /* multi-segment files the host had to gather as a whole (full marker walks) */
} jpgpu_ingest_stats;
int jpgpu_batch_ingest_stats(const jpgpu_batch *b, jpgpu_ingest_stats *stats);
/* ---- (1b) files that are in device memory already: jpgpu_batch_upload without the host link.
 * device_jpeg[i] is device memory of the context's device that holds the len[i] bytes of file i, whole, at any byte address.
 * THE FILES ARE COPIED (jpgpu_batch_upload's contract, not the encoder's 4c): when the call returns the batch owns a copy of
 * every file in its input buffer, the caller may overwrite or free its memory, and every later call on the batch
 * (jpgpu_batch_decode, the stage calls, _result, the _download_ calls, the re-plans and the partial flush of progressive files)
 * behaves as it does behind a host upload of the same bytes.  No kernel reads the caller's memory after the call, and none
 * reads outside [device_jpeg[i], device_jpeg[i] + len[i]) during it.
 * What crosses the host link: of every file its head -- the bytes up to the end of its first SOS header plus
 * JPGPU_DEVICE_HEAD_PAD, at most 64 KiB; a device-side walk over the marker segments finds that length, and all 64 KiB are
 * taken where the walk meets anything it does not expect (the host parses what it gets, no result depends on the walk) -- and,
 * whole, the files that need the full marker walks on the host (jpgpu_ingest_stats.n_full_walk: several scans, progressive,
 * bytes behind the EOI, truncated data, a first scan that starts behind the head).  The gather, the walk and the verdict run
 * as a fixed number of launches and copies per upload on the context's upload stream.
 * Ordering: like every upload it is ordered behind device work this batch has issued and not yet synchronised; the work that
 * PRODUCED the bytes must be complete -- or ordered before the context's upload stream -- when this call is made.
 * JPGPU_ERR_ARGUMENT for the whole call, decided here and before anything is enqueued, leaving the batch empty
 * (jpgpu_batch_size = 0): a NULL batch or array; a NULL file pointer with len[i] != 0; a pointer hipPointerGetAttributes does
 * not report as device memory of the context's device (host, pinned host and managed memory are refused); a file whose len[i]
 * bytes do not lie inside ONE allocation (hipMemGetAddressRange); an unknown format.  len[i] == 0 is the empty file: it gets the
 * host path's per-image status and its pointer is not looked at. */
#define JPGPU_DEVICE_HEAD_PAD 64
int jpgpu_batch_upload_device(jpgpu_batch *b, const void *const *device_jpeg, const size_t *len, int n, int format);
/* What the last jpgpu_batch_upload_device moved (all zero behind any other upload of the batch, and behind a refused one); jpgpu_batch_ingest_stats keeps reporting
 * the plans and the times (n_pinned_dma = 0).  Compare jpgpu_sizeof_device_ingest_stats() with sizeof at load time. */
typedef struct jpgpu_device_ingest_stats {
    int32_t files_gathered;    /* files copied from the caller's device memory into the input buffer */
    int32_t files_downloaded;  /* files fetched whole to the host for the full marker walks */
    int32_t walker_giveups;    /* files whose head is min(len, 64 KiB) because the device-side walk gave up */
    float gather_ms;           /* device time of the gather (events around it on the upload stream) */
    uint64_t bytes_gathered;
    uint64_t head_bytes;       /* D2H: the packed heads, each rounded up to 16 bytes (beside 12 bytes per file of lengths and offsets) */
    uint64_t bytes_downloaded; /* D2H: the files of files_downloaded */
} jpgpu_device_ingest_stats;
size_t jpgpu_sizeof_device_ingest_stats(void);
int jpgpu_batch_device_ingest_stats(const jpgpu_batch *b, jpgpu_device_ingest_stats *stats);
/* How the last upload planned the entropy stage of its sequential scans (read only; for tests and tools).  K2 = scans with
 * restart intervals: workgroups of the plain list, and runs of adjacent scans with the same tables and geometry POOLED into
 * chunks of 64 intervals (at most 8 pools).  K2S = scans without restart intervals: the final pass's plain list and its pools
 * (at most 8), and the distinct table sets among those scans. */
typedef struct jpgpu_plan_stats {
    int32_t k2_plain_work;      /* entries (workgroups) of K2's plain list */
    int32_t k2_pools;           /* pooled runs of K2 */
    int32_t k2_pooled_chunks;   /* chunks of 64 restart intervals over all K2 pools */
    int32_t huffman_waves;      /* waves per K2 workgroup (what the batch's largest table set leaves room for) */
    int32_t k2s_scans;          /* scans decoded by K2S */
    int32_t k2s_plain_work;     /* entries of the K2S final pass's plain list */
    int32_t k2s_pools;          /* pooled runs of the K2S final pass */
    int32_t k2s_table_sets;     /* distinct table sets among the K2S scans */
    int32_t k2s_subs_per_lane;  /* subsequences a lane of the K2S final pass takes */
    int32_t k2s_sub_shift;      /* log2 of the subsequence length in bits the upload used; 0 without K2S scans */
    int32_t k2s_subs;           /* subsequences over all K2S scans of the upload */
} jpgpu_plan_stats;
/* sizeof(jpgpu_plan_stats) as THIS library writes it. */
size_t jpgpu_sizeof_plan_stats(void);
int jpgpu_batch_plan_stats(const jpgpu_batch *b, jpgpu_plan_stats *stats);
/* How the last upload planned K3 (read only; for tests and tools): work entries (workgroups) per output layout class -- generic,
 * YCbCr 1x1 / 2x1 / 2x2, gray, store holding samples.  Scans ordered behind other scans of their image are not counted.
 * n must be JPGPU_IDCT_LAYOUT_CLASSES. */
#define JPGPU_IDCT_LAYOUT_CLASSES 6
int jpgpu_batch_idct_work(const jpgpu_batch *b, int32_t *counts, int n);
/* ... and how many of them belong to scans the planner hands over to K3 as half-line planes (the split form of the class's kernel). */
int jpgpu_batch_idct_split_work(const jpgpu_batch *b, int32_t *counts, int n);

/* Windows: decode a rectangle of each image.  A window is given in pixels of the frame; the batch decodes image i into an output the size
 * of its window, and the output stage (K3) transforms and stores only the MCUs the window touches.  The entropy stage decodes the whole
 * scan: jpgpu_batch_result is field for field what it is without windows, and jpgpu_batch_download_coefficients /
 * jpgpu_batch_coefficients_device return the whole frame's coefficients.
 *   Pixels.  For every whole-pixel format (INTERLEAVED_U8, INTERLEAVED_U8_SCALED, RGB_U8, RGBA_U8, RGB_PLANAR_U8 / _F16 / _F32) the window's
 * output equals, sample for sample, the slice [y : y + height, x : x + width] of what the same upload produces without windows -- images
 * that fail or end early (unreached samples read zero in both), progressive frames and the partial flush of a failing one, multi-scan
 * frames and an image that is planned again on its own included.  The affine constants of the float formats apply unchanged.
 *   Geometry.  jpgpu_image_info.width / height stay the frame's; out_bytes and plane[] describe the window: (H, W, C) formats hold
 * height * width * C bytes with pitch width; RGB_PLANAR_* three tight planes of width x height samples, plane[c] = {c * width * height *
 * sizeof(T), width, height, width}.  out_offset stays a multiple of 256.
 *   jpgpu_batch_set_windows gives the windows of the NEXT upload of this batch (jpgpu_batch_upload, _upload_segments, _upload_device),
 * image i -> windows[i]; {0, 0, 0, 0} = the whole frame.  They are consumed by that upload, accepted or refused: the one after it decodes
 * whole frames again unless the call is repeated.  n == 0 (windows may be NULL) withdraws pending windows.  JPGPU_ERR_ARGUMENT for a NULL
 * batch, n < 0, or NULL windows with n > 0.
 *   An upload with pending windows returns JPGPU_ERR_ARGUMENT, decided before anything is enqueued and leaving the batch empty
 * (jpgpu_batch_size = 0), when its n differs from the windows' n, or when its format is not a whole-pixel format (PLANAR_U8, PLANAR_I16
 * and EXTENDED_U16 have MCU-padded component planes or another geometry); jpgpu_batch_upload_frames with pending windows is refused the
 * same way.
 *   A window that does not lie inside the frame (x + width > W or y + height > H), or with exactly one of width and height zero, fails
 * that image alone: JPGPU_ERR_ARGUMENT / JPGPU_DETAIL_NONE, out_bytes = 0; the other images are not affected.  An image whose headers
 * fail keeps the status it has without windows.
 *   The fast layout classes of K3 serve a window whose x is a multiple of the MCU width and whose width satisfies the class's rule for a
 * frame's width (RGB_U8 and RGB_PLANAR_*); y and height are free.  Any other window takes the generic class.
 *   Not windowed: jpgpu_decoder_*, jpgpu_decode_scan, jpgpu_progressive_*, jpgpu_multi_*. */
typedef struct jpgpu_rect {
    uint32_t x, y, width, height; /* pixels of the frame; {0, 0, 0, 0} = the whole frame */
} jpgpu_rect;
size_t jpgpu_sizeof_rect(void);
int jpgpu_batch_set_windows(jpgpu_batch *b, const jpgpu_rect *windows, int n);
/* The window image i was planned with ({0, 0, W, H} for a whole frame).  Valid after an upload. */
int jpgpu_batch_image_window(const jpgpu_batch *b, int i, jpgpu_rect *window);
/* Sum of n_mcus over every K3 work entry the last upload listed (all classes, all levels; read only, for tests and tools). */
int jpgpu_batch_idct_listed_mcus(const jpgpu_batch *b, uint64_t *mcus);

/* ---- Colour: CMYK, YCCK and Adobe-RGB files under the RGB formats (an extension beyond the reference, whose callers refuse such files).
 *   By default (JPGPU_COLOR_YCC) the RGB formats treat every 1-component frame as grey and every 3-component frame as YCbCr, and refuse
 * every other frame.  Under JPGPU_COLOR_FILE an image is converted by what its file declares.  The kind of an image of 8-bit precision is
 * libjpeg's rule over the markers between SOI and the first SOS -- "JFIF seen": an APP0 whose payload (behind the length) is at least 14
 * bytes and begins "JFIF\0"; "Adobe seen": an APP14 whose payload is at least 12 bytes and begins "Adobe", its transform = payload[11],
 * the last such segment counting:
 *     1 component    GRAY
 *     3 components   JFIF seen: YCBCR.  Else Adobe seen: transform 0 RGB, any other YCBCR.  Else component ids 'R', 'G', 'B': RGB.
 *                    Otherwise YCBCR.
 *     4 components   Adobe seen with transform 0: CMYK; with any other transform: YCCK.  No Adobe: CMYK.  JFIF is ignored.
 *     2 or more than 4 components, or a precision other than 8: refused as without the policy.
 *   Pixels.  With s0..s3 the INTERLEAVED_U8 ("O2") bytes of the pixel and d(x) = (x + 128 + ((x + 128) >> 8)) >> 8, which is x / 255
 * rounded to nearest for 0 <= x <= 65025:
 *     GRAY, YCBCR    the bytes the format holds without the policy
 *     RGB            (R, G, B) = (s0, s1, s2)
 *     CMYK           R = d(s0 * s3), G = d(s1 * s3), B = d(s2 * s3)      (Adobe files store inverted inks; Pillow's CMYK -> RGB)
 *     YCCK           (r, g, b) = RGB_U8's conversion of (s0, s1, s2), the same tables; R = d((255 - r) * s3), likewise G and B
 * RGBA_U8 adds A = 255; RGB_PLANAR_U8 holds the same bytes as planes; RGB_PLANAR_F16 / _F32 apply their affine step to these bytes (one
 * float32 multiply, one float32 add, never fused).  Windows and the resize stage see these bytes like any others.
 *   Only RGB_U8, RGBA_U8 and RGB_PLANAR_U8 / _F16 / _F32 read the policy; every other format decodes and reports as without it.
 * jpgpu_image_info.out_bytes stays 3 (RGBA_U8: 4) samples per pixel; out_offset of the image BEHIND a 4-component image may lie further on
 * than out_bytes suggests (the image's samples pass through a scratch slot of 4 bytes per pixel at the same offset): use out_offset.
 *   jpgpu_batch_set_color_policy is state of the batch: every later upload reads it until it is set again (it is not consumed the way
 * windows are).  JPGPU_ERR_ARGUMENT for a NULL batch or an unknown value.  jpgpu_batch_upload_frames applies the rule with no marker seen.
 *   Not covered: jpgpu_decoder_*, jpgpu_decode_scan, jpgpu_progressive_*, jpgpu_multi_* (they decode as JPGPU_COLOR_YCC). */
typedef enum jpgpu_color_policy {
    JPGPU_COLOR_YCC = 0, /* 1 component = grey, 3 = YCbCr, anything else refused by the RGB formats */
    JPGPU_COLOR_FILE = 1 /* what the file declares */
} jpgpu_color_policy;
typedef enum jpgpu_color_kind {
    JPGPU_COLOR_KIND_GRAY = 0,
    JPGPU_COLOR_KIND_YCBCR = 1,
    JPGPU_COLOR_KIND_RGB = 2,
    JPGPU_COLOR_KIND_CMYK = 3,
    JPGPU_COLOR_KIND_YCCK = 4
} jpgpu_color_kind;
int jpgpu_batch_set_color_policy(jpgpu_batch *b, int policy);
/* The kind image i was planned with: GRAY or YCBCR under JPGPU_COLOR_YCC and under a format that does not read the policy, YCBCR for an
 * image that failed at upload.  Valid after an upload; JPGPU_ERR_ARGUMENT for a NULL argument or an index out of range. */
int jpgpu_batch_image_color(const jpgpu_batch *b, int i, int *kind);
/* The rule above on a file's headers.  Host only, no context needed.  The library's usual header errors (jpgpu_status) for a file without
 * a frame header or with broken headers; JPGPU_ERR_NOT_SUPPORTED for a frame the rule refuses; JPGPU_ERR_ARGUMENT for a NULL argument. */
int jpgpu_identify_color(const uint8_t *file, size_t len, int *kind);

/* ---- Orientation: the Exif orientation of a file, or a flip or turn the caller asks for, applied in the output stage (an extension beyond the
 * reference, whose callers hand the stored samples on).
 *   By default (JPGPU_ORIENT_STORED) an image comes out as its file stores it.  Under JPGPU_ORIENT_FILE it is turned the way its Exif block
 * says, as ImageOps.exif_transpose, torchvision's apply_exif_orientation and the browsers do.  The rule.  The block is the FIRST APP1 between
 * SOI and the first SOS whose payload begins "Exif\0\0"; only that segment is read.  With t the bytes behind those six: t[0:2] is "II"
 * (little-endian) or "MM" (big-endian), the uint16 at t + 2 is 42, the uint32 at t + 4 is the offset o of IFD0, the uint16 at t + o its entry
 * count, the 12-byte entries follow from t + o + 2.  The first entry with tag 0x0112 counts: of type 3 (SHORT) and count 1, its value is the
 * uint16 at entry + 8 in the file's byte order, and a value of 1..8 is the orientation.  No such segment, another magic, a read that would
 * leave the segment, another type or count, a value of 0 or above 8, no such tag: orientation 1.  A bad block never fails an image.
 *   The transform.  With H x W the stored frame and (Y, X) a pixel of the output, the source pixel (y, x) is
 *     1   H x W   (Y, X)                        5   W x H   (X, Y)              transpose
 *     2   H x W   (Y, W-1-X)        mirror      6   W x H   (H-1-X, Y)          a quarter turn clockwise
 *     3   H x W   (H-1-Y, W-1-X)    half turn   7   W x H   (H-1-X, W-1-Y)      transverse
 *     4   H x W   (H-1-Y, X)        flip        8   W x H   (X, W-1-Y)          a quarter turn counter-clockwise
 * and every sample of the output is, bit for bit, the sample at (y, x) of what the same upload produces under orientation 1 -- for images
 * that fail or end early, for progressive frames and their partial flush, for every colour kind under JPGPU_COLOR_FILE, and for the float
 * formats, whose affine step is per sample.
 *   jpgpu_batch_set_orientation_policy is state of the batch like the colour policy.  jpgpu_batch_set_orientations gives the NEXT upload of
 * whole files one value per file and is consumed by it like windows: 1..8 is used as given, whatever the file says; 0 leaves the image to the
 * policy; n == 0 withdraws a pending list.  JPGPU_ERR_ARGUMENT for a value above 8; an upload whose n differs from the list's is refused with
 * JPGPU_ERR_ARGUMENT and leaves the batch empty, and so is jpgpu_batch_upload_frames while a list is pending.
 *   Only RGB_U8, RGBA_U8 and RGB_PLANAR_U8 / _F16 / _F32 read orientation; every other format decodes as stored and reports 1, and an upload
 * under one of them with a list pending is refused like windows under PLANAR_U8.
 *   Geometry.  jpgpu_image_info.width / height stay the stored frame's; out_bytes and plane[] describe the oriented output, width and height
 * swapped for 5..8.  Windows (jpgpu_batch_set_windows) are given in pixels of the ORIENTED frame, which is what the caller sees: the windowed
 * output is that slice of the oriented whole decode, jpgpu_batch_image_window returns the rectangle as given, and a window outside the
 * oriented frame fails that image alone.  The resize stage reads the oriented image.  out_offset of the image behind an oriented one follows
 * the rule of the colour kinds (the samples pass through a scratch slot at the same offset): use out_offset.
 *   Not covered: jpgpu_decoder_*, jpgpu_decode_scan, jpgpu_progressive_*, jpgpu_multi_* (they decode as stored). */
typedef enum jpgpu_orientation_policy {
    JPGPU_ORIENT_STORED = 0, /* as the file stores the pixels */
    JPGPU_ORIENT_FILE = 1    /* as the file's Exif orientation says */
} jpgpu_orientation_policy;
int jpgpu_batch_set_orientation_policy(jpgpu_batch *b, int policy);
int jpgpu_batch_set_orientations(jpgpu_batch *b, const uint8_t *orientations, int n);
/* The orientation image i was planned with: 1 under a format that does not read it and for an image that failed at upload.  Valid after an
 * upload; JPGPU_ERR_ARGUMENT for a NULL argument or an index out of range. */
int jpgpu_batch_image_orientation(const jpgpu_batch *b, int i, int *orientation);
/* The rule above on a file's headers.  Host only, no context needed.  The library's usual header errors (jpgpu_status) for a file without a
 * frame header or with broken headers -- never for a broken Exif block; JPGPU_ERR_ARGUMENT for a NULL argument. */
int jpgpu_identify_orientation(const uint8_t *file, size_t len, int *orientation);

/* ---- Chroma upsampling: libjpeg's "fancy" (triangle) filter in place of the reference's sample replication, applied in the output stage (an
 * extension beyond the reference; the switch DALI and nvJPEG call fancy_upsampling).
 *   By default (JPGPU_UPSAMPLE_REPLICATE) a sub-sampled chroma sample is repeated over the pixels it covers, as the reference does, bit for
 * bit as before.  Under JPGPU_UPSAMPLE_FANCY an image is FILTERED when all of these hold: its colour kind is YCbCr (a three-component frame
 * under JPGPU_COLOR_YCC, kind YCBCR under JPGPU_COLOR_FILE); its precision is 8; component 0 carries the frame's maximal sampling factors;
 * components 1 and 2 have equal factors and (hs, vs) = (Hmax / H1, Vmax / V1) is (2, 1), (2, 2) or (1, 2); and, for hs == 2, the chroma plane
 * is more than two samples wide, cw = ceil(W / 2) > 2 (libjpeg takes its replicating routine for narrower planes).  Every other image --
 * grey, 4:4:4, 4:1:1 and other ratios, the RGB, CMYK and YCCK kinds, other precisions -- decodes exactly as under REPLICATE.
 *   The function.  With I the INTERLEAVED_U8 decode of the same file (stored orientation, whole frame), the native chroma samples are
 * C_c[j][i] = I[j * vs][i * hs][c] for c = 1, 2, i < cw = ceil(W / hs), j < ch = ceil(H / vs); indices clamp to that REAL extent, never to
 * the MCU padding; luma is I[y][x][0], unchanged.  For pixel (x, y), in integers:
 *     vertical (vs == 2):    j = y >> 1; jf = j - 1 for even y, j + 1 for odd y, clamped; s[i] = 3 * C[j][i] + C[jf][i]; rb = 1 for even y, 2 for odd
 *     horizontal (hs == 2):  i = x >> 1; in = i - 1 for even x, i + 1 for odd x, clamped
 *     h2v1:  (3 * C[y][i] + C[y][in] + (x even ? 1 : 2)) >> 2
 *     h1v2:  (s[x] + rb) >> 2
 *     h2v2:  (3 * s[i] + s[in] + (x even ? 8 : 7)) >> 4
 * which is libjpeg's h2v1 / h2v2 / h1v2 fancy upsampler, its special first and last columns included.  The output sample is what the
 * format's own path makes of (Y, Cb', Cr'): the RGB_U8 conversion, then the alpha byte, the plane split and the per-sample affine step of the
 * float forms.  Everything behind it composes on the filtered picture: a window is that slice of the filtered whole decode, bit for bit; an
 * orientation turns it; the resize stage resamples it; a file that fails gives the filter of its partial picture.
 *   Only RGB_U8, RGBA_U8 and RGB_PLANAR_U8 / _F16 / _F32 read the policy; every other format decodes as before.  The policy is state of the
 * batch like the colour policy: every later upload of whole files reads it until it is set again.  Sizes, planes and out_bytes are what
 * REPLICATE reports; out_offset of the image behind a filtered one follows the rule of the colour kinds: use out_offset.
 *   Not claimed: equality with libjpeg's RGB.  The IDCT here is the reference's float one and the colour arithmetic the reference's, not
 * libjpeg's integer IDCT, fixed-point conversion or merged upsampling; YCCK chroma stays replicated.
 *   Not covered: jpgpu_decoder_*, jpgpu_decode_scan, jpgpu_progressive_*, jpgpu_multi_*, jpgpu_batch_upload_frames (they replicate). */
typedef enum jpgpu_upsampling_policy {
    JPGPU_UPSAMPLE_REPLICATE = 0, /* the reference's sample replication */
    JPGPU_UPSAMPLE_FANCY = 1      /* libjpeg's triangle filter for h2v1, h2v2 and h1v2 YCbCr images */
} jpgpu_upsampling_policy;
/* JPGPU_ERR_ARGUMENT for any other value. */
int jpgpu_batch_set_upsampling_policy(jpgpu_batch *b, int policy);
/* 1 where image i was planned with the filter, else 0 (an image the rule leaves replicated, a format that does not read the policy, an
 * image that failed at upload).  Valid after an upload; JPGPU_ERR_ARGUMENT for a NULL argument or an index out of range. */
int jpgpu_batch_image_upsampling(const jpgpu_batch *b, int i, int *applied);
/* Measuring aid.  Device time of the last call of the upsampling kernels (K3U) of this upload, from an event pair of its own (synchronises).
 * The pair is recorded only for an upload made while the environment holds JPGPU_TIME_UPSAMPLE=1, so that no other decode pays for it;
 * JPGPU_ERR_INVALID_OPERATION otherwise, and when the upload has no filtered image or has not been decoded. */
int jpgpu_batch_upsampling_ms(jpgpu_batch *b, float *ms);

/* ---- Grey output: ONE plane per image in place of three (an extension beyond the reference; torchvision's ImageReadMode.GRAY, the Y output
 * format of nvJPEG and rocJPEG, libjpeg's JCS_GRAYSCALE).
 *   By default (JPGPU_CHANNELS_RGB) every format decodes as before, bit for bit.  Under JPGPU_CHANNELS_LUMA the formats RGB_PLANAR_U8 / _F16 /
 * _F32 deliver one tight plane of the oriented frame, or of its window: out_bytes = W * H * sizeof(sample), plane[0] = {0, W, H, W},
 * plane[1] and plane[2] zero.  The float forms use scale[0] and bias[0] of jpgpu_batch_set_output_affine with the arithmetic of the three
 * planes.  out_offset stays a multiple of 256; use it, as under the colour policy.
 *   The sample of pixel (x, y):
 *     kinds GRAY and YCBCR   the byte INTERLEAVED_U8 holds at channel 0 of that pixel: component 0's sample.  No chroma is read, so the
 *                            upsampling policy has no effect: jpgpu_batch_image_upsampling says 0 for every image.
 *     kinds RGB, CMYK, YCCK  (these exist only under JPGPU_COLOR_FILE)  (19595 * R + 38470 * G + 7471 * B + 32768) >> 16  with R, G, B the
 *                            bytes RGB_U8 holds for that pixel under the colour policy: Pillow's convert("L").
 * Windows, orientation (the plane is turned like the three planes are), the partial picture of a failing file and the per-image refusals are
 * those of the RGB formats; an image that failed reads as zeros.
 *   Two roads, chosen per image (jpgpu_batch_luma_work counts them).  The FAST road transforms component 0's blocks alone, straight from the
 * coefficient store: kind GRAY or YCBCR, precision 8, orientation 1, one sequential scan that holds every frame component once with frame
 * component 0 first, component 0 carrying the frame's maximal sampling factors (vertically it may also have one block per MCU column
 * under a taller MCU, as (2, 1) luma beside (1, 2) chroma has: its rows are repeated like the reference repeats them), and no caller's
 * canvas.  The other components' factors, the width, the height and the window are free.  Everything else -- progressive and multi-scan frames, the kinds RGB, CMYK and YCCK,
 * orientations 2..8 -- takes the SCRATCH road: the INTERLEAVED_U8 samples of the stored window, then one kernel that forms the sample
 * and turns the plane.  The bytes do not depend on the road.
 *   Only RGB_PLANAR_U8 / _F16 / _F32 read the policy; every other format decodes as before.  It is state of the batch like the colour
 * policy: every later upload of whole files reads it until it is set again.
 *   The resize stage (jpgpu_batch_set_resize) over a LUMA upload of RGB_PLANAR_U8 resamples the one plane with the same tap tables and the
 * same function per plane, scale[0] and bias[0]: the buffer is T[n][1][out_height][out_width], and jpgpu_batch_resized_device and
 * jpgpu_batch_download_resized count one plane per image.
 *   Not covered: jpgpu_decoder_*, jpgpu_decode_scan, jpgpu_progressive_*, jpgpu_multi_*, jpgpu_batch_upload_frames (three planes, as
 * before); a fast road for turned images or from the split hand-off; an interleaved [H, W, 1] form; grey by any other formula. */
typedef enum jpgpu_channels_policy {
    JPGPU_CHANNELS_RGB = 0, /* three planes, as before */
    JPGPU_CHANNELS_LUMA = 1 /* one plane: component 0's samples, or L of the file's RGB */
} jpgpu_channels_policy;
/* JPGPU_ERR_ARGUMENT for any other value. */
int jpgpu_batch_set_channels_policy(jpgpu_batch *b, int policy);
/* 1 where image i was planned with one plane, else 3 (the channels of the RGB formats; the policy unset, a format that does not read it, an
 * image that failed at upload).  Valid after an upload; JPGPU_ERR_ARGUMENT for a NULL argument or an index out of range. */
int jpgpu_batch_image_channels(const jpgpu_batch *b, int i, int *channels);
/* counts[0] = images of this upload planned on the fast road, counts[1] = on the scratch road.  Valid after an upload. */
int jpgpu_batch_luma_work(const jpgpu_batch *b, int32_t counts[2]);

/* ---- Arithmetic: the transform and the colour constants of libjpeg in place of the reference's (an extension beyond the reference; what
 * Pillow, torchvision and OpenCV deliver, all on libjpeg-turbo's jpeg_idct_islow).
 *   By default (JPGPU_ARITHMETIC_REFERENCE) every format decodes as before, bit for bit.  Under JPGPU_ARITHMETIC_LIBJPEG the five RGB formats
 * (RGB_U8, RGBA_U8, RGB_PLANAR_U8 / _F16 / _F32) change in two places; every other format ignores the policy.
 *   1. THE TRANSFORM, per image (jpgpu_batch_image_arithmetic says which one an image took).  For every 8 x 8 block, with coef[k] its int16
 * coefficients and q[k] the uint16 quantisers of its component:
 *       d[k] = (int32)coef[k] * (int32)q[k]                                     (int16 x uint16: no overflow)
 *     then libjpeg's jidctint.c, CONST_BITS = 13, PASS1_BITS = 2, on the eight values d0..d7 of each COLUMN first, then of each ROW of the
 *     workspace the columns left:
 *       z1 = (d2 + d6) * 4433      e2 = z1 - d6 * 15137       e3 = z1 + d2 * 6270       e0 = (d0 + d4) << 13       e1 = (d0 - d4) << 13
 *       t10 = e0 + e3    t13 = e0 - e3    t11 = e1 + e2    t12 = e1 - e2
 *       t0 = d7   t1 = d5   t2 = d3   t3 = d1       z1 = t0 + t3   z2 = t1 + t2   z3 = t0 + t2   z4 = t1 + t3     z5 = (z3 + z4) * 9633
 *       t0 *= 2446   t1 *= 16819   t2 *= 25172   t3 *= 12299     z1 *= -7373   z2 *= -20995   z3 = z3 * -16069 + z5   z4 = z4 * -3196 + z5
 *       t0 += z1 + z3    t1 += z2 + z4    t2 += z2 + z3    t3 += z1 + z4
 *       out0, out7 = t10 +- t3     out1, out6 = t11 +- t2     out2, out5 = t12 +- t1     out3, out4 = t13 +- t0
 *     each out descaled: (x + 1024) >> 11 behind the columns, (x + 131072) >> 18 behind the rows.  The sample is clamp(v + 128, 0, 255).
 *     Every sum, product and left shift is 32-bit two's complement and WRAPS; the two descales are arithmetic right shifts of the wrapped
 *     value.  The clamp is what libjpeg's SIMD code does (it saturates); its C code reads a table that wraps at +-512 around the centre.
 *     Equality with libjpeg is claimed where every dequantised coefficient and workspace value fits int16 and every pass sum fits int32 --
 *     every file an encoder made --; outside that range the function above is what is pinned.
 *     An image takes it if its frame precision is 8, it has 1, 3 or 4 components as its colour kind has, every scan of it has at most 16
 *     blocks per MCU and components that are replicated by 1, 2 or 4 in each direction, no two of its sequential scans write the same
 *     component and no scan names a component twice, no sequential component has several blocks per MCU line or column that are replicated as
 *     well, and its progressive frame, if it is one, is not the kind whose Dispose() the reference runs slot by slot.  Every other image
 *     keeps the reference's float transform.  So does the second issue of a progressive file that failed, whose pixels are not defined.
 *   2. THE COLOUR CONSTANTS, per upload: every YCbCr -> RGB step of the decode (YCCK's inner one too) takes libjpeg's
 *     R = Y + (91881 * Cr + 32768 >> 16), B = Y + (116130 * Cb + 32768 >> 16), G = Y + (-22554 * Cb - 46802 * Cr + 32768 >> 16)
 *     in place of the reference's, which differ in one constant (-22553).  The CMYK product and the grey formula of JPGPU_CHANNELS_LUMA stay.
 *   Chroma upsampling stays its own policy: JPGPU_ARITHMETIC_LIBJPEG alone keeps replication; with JPGPU_UPSAMPLE_FANCY the pixels are
 * libjpeg's default output.  Windows, the colour policy, orientation, grey output, the float samples and the resize stage compose: an image
 * that takes the transform goes through the scratch image like a filtered one, and everything behind it reads its samples.
 *   State of the batch like the colour policy: every later upload of whole files reads it until it is set again.
 *   Not covered: jpgpu_decoder_*, jpgpu_decode_scan, jpgpu_progressive_*, jpgpu_multi_*, jpgpu_batch_upload_frames (the reference's arithmetic,
 * as before); libjpeg's other transforms (ifast, float; the scaled ones are "Scaled decode" below); 12-bit frames. */
typedef enum jpgpu_arithmetic_policy {
    JPGPU_ARITHMETIC_REFERENCE = 0, /* the reference's float transform and constants, as before */
    JPGPU_ARITHMETIC_LIBJPEG = 1    /* jpeg_idct_islow and libjpeg's colour constants */
} jpgpu_arithmetic_policy;
/* JPGPU_ERR_ARGUMENT for any other value. */
int jpgpu_batch_set_arithmetic_policy(jpgpu_batch *b, int policy);
/* JPGPU_ARITHMETIC_LIBJPEG where image i was planned with the integer transform, else JPGPU_ARITHMETIC_REFERENCE (the policy unset, a format
 * that does not read it, an image outside the rule above, an image that failed at upload).  Valid after an upload; JPGPU_ERR_ARGUMENT for a
 * NULL argument or an index out of range. */
int jpgpu_batch_image_arithmetic(const jpgpu_batch *b, int i, int *arithmetic);

/* ---- Scaled decode: the picture at 1/2, 1/4 or 1/8 size with libjpeg's reduced transforms (an extension beyond the reference; libjpeg's
 * scale_num / scale_denom, which Pillow reaches through Image.draft(), OpenCV through IMREAD_REDUCED_COLOR_2/4/8).  It is part of the
 * arithmetic of libjpeg: an image takes a denominator above 1 exactly where it takes the integer transform above
 * (jpgpu_batch_image_arithmetic says JPGPU_ARITHMETIC_LIBJPEG).  Everything else keeps full size and reports 1: the policy
 * JPGPU_ARITHMETIC_REFERENCE, a format that does not read the arithmetic policy, 12-bit frames and the odd layouts of the rule above, and
 * every entry the arithmetic policy does not cover.
 *   Let m = 8 / denom: 4, 2 or 1.
 *   OUTPUT SIZE.  W' = ceil(W * m / 8), H' = ceil(H * m / 8).
 *   PER-COMPONENT TRANSFORM SIZE (jdmaster.c of library version 62).  A component with factors h, v under the frame's maxima hmax, vmax:
 *       s = m;  while (s < 8 && (hmax * m) % (h * s * 2) == 0 && (vmax * m) % (v * s * 2) == 0) s *= 2;
 *     Its block yields s x s samples; the replication left is rh = hmax * m / (h * s), rv = vmax * m / (v * s).  4:2:0 at 1/2, 1/4, 1/8:
 *     luma 4, 2, 1 and chroma 8, 4, 2 with nothing left to replicate; 4:4:4 and grey: s = m; 4:2:2: s = m for all, rh = 2 stays for chroma.
 *   BLOCK TRANSFORMS (jidctred.c).  d[r][c] = (int32)coef * (int32)q, CONST_BITS = 13, PASS1_BITS = 2, DESCALE(x, n) = (x + 2^(n-1)) >> n
 *     arithmetic; every sum, product and left shift is 32-bit two's complement and wraps, as above; the sample is clamp(v + 128, 0, 255).
 *     s = 8: jpeg_idct_islow, as above.
 *     s = 4 (jpeg_idct_4x4): pass 1 over columns 0..3 and 5..7 (column 4 is never used) on rows 0, 1, 2, 3, 5, 6, 7:
 *       t0 = d0 << 14     t2 = d2 * 15137 - d6 * 6270     t10 = t0 + t2     t12 = t0 - t2
 *       a = -d7 * 1730 + d5 * 11893 - d3 * 17799 + d1 * 8697          b = -d7 * 4176 - d5 * 4926 + d3 * 7373 + d1 * 20995
 *       out0..3 = DESCALE(t10 + b), DESCALE(t12 + a), DESCALE(t12 - a), DESCALE(t10 - b)      by 12 bits;
 *       pass 2 the same on each of the 4 workspace rows over workspace columns 0, 1, 2, 3, 5, 6, 7, by 19 bits.
 *     s = 2 (jpeg_idct_2x2): pass 1 over columns 0, 1, 3, 5, 7 on rows 0, 1, 3, 5, 7:
 *       t10 = d0 << 15     t0 = -d7 * 5906 + d5 * 6967 - d3 * 10426 + d1 * 29692     out0, out1 = DESCALE(t10 + t0), DESCALE(t10 - t0)  by 13 bits;
 *       pass 2 the same on each of the two workspace rows over workspace columns 0, 1, 3, 5, 7, by 20 bits.
 *     s = 1: DESCALE(d[0][0], 3).
 *     (libjpeg's shortcut for a column without AC terms gives the same values.)
 *   ASSEMBLY.  The block at block position (bx, by) of its component's plane lands at (bx * s * rh, by * s * rv) of the reduced picture,
 *     every sample repeated rh x rv times, the picture clipped to W' x H'.
 *   UPSAMPLING.  The reduced picture is an ordinary picture whose chroma ratio is (rh, rv).  Under JPGPU_UPSAMPLE_FANCY the rule of "Chroma
 *     upsampling" applies to it unchanged where (rh, rv) is (2,1), (2,2) or (1,2) and denom < 8 (libjpeg switches the filter off where the
 *     smallest s is 1); the chroma extent is ceil(W' / rh), ceil(H' / rv).  Otherwise chroma is replicated.
 *   Colour, orientation, grey output, the float samples and the resize stage run behind this on the reduced picture as they run behind the
 *   integer transform.  WINDOWS are in pixels of the reduced (and, if turned, oriented) frame.  jpgpu_batch_image_info's width / height stay
 *   the frame's; plane[], out_bytes and jpgpu_batch_image_window describe the reduced picture.
 *   Equality with libjpeg is claimed under the condition stated above: dequantised and workspace values inside int16, pass sums inside int32.
 *   State of the batch like the arithmetic policy: every later upload of whole files reads it until it is set again. */
/* denom: 1 (the default), 2, 4 or 8; JPGPU_ERR_ARGUMENT for anything else. */
int jpgpu_batch_set_scale_policy(jpgpu_batch *b, int denom);
/* Pillow's draft() rule, per image: with k = min(w / min_w, h / min_h) in integer division over the image's ORIENTED frame w x h, the
 * denominator is 8 if k >= 8, else 4 if k >= 4, else 2 if k >= 2, else 1 -- the smallest picture that is still at least min_w x min_h.
 * While set it overrides the scale policy; (0, 0) switches it off.  JPGPU_ERR_ARGUMENT where only one of the two is 0. */
int jpgpu_batch_set_scale_fit(jpgpu_batch *b, uint32_t min_w, uint32_t min_h);
/* The denominator image i was planned with: 1, 2, 4 or 8 (1 for an image that failed at upload).  Valid after an upload;
 * JPGPU_ERR_ARGUMENT for a NULL argument or an index out of range. */
int jpgpu_batch_image_scale(const jpgpu_batch *b, int i, int *denom);

/* Coefficient hand-off for multi-scan (progressive, SOF2) images -- BASELINE config 5's "coefficient accumulate then single
 * IDCT pass": the caller's progressive entropy decoder accumulates the coefficient store, the GPU runs what
 * JpegHuffmanProgressiveScanDecoder.Dispose (ScanDecoder/JpegHuffmanProgressiveScanDecoder.cs:421-470: dequantise, IDCT,
 * level shift over the MCU grid) and JpegBlockAllocator.Flush (JpegBlockAllocator.cs:120-190) do.  Images are described
 * by their frame header and quantisation tables only (qt[i][tq][64], zig-zag order); then
 * jpgpu_batch_upload_coefficients(i, blocks in MCU scan order: MCU raster, component order, block raster in the MCU)
 * and jpgpu_batch_run_idct. */
int jpgpu_batch_upload_frames(jpgpu_batch *b, const jpgpu_frame *frames, const uint16_t *qt, int n, int format);

/* Launches the device pipeline on the ctx stream (asynchronous):
 *   marker index -> Huffman MCU decode (ref: ...BaselineScanDecoder.cs:51-222) ->
 *   dequantise + float32 IDCT + level shift (ref: ScanDecoder/JpegScanDecoder.cs:50-73, FastFloatingPointDCT.cs:54-185) ->
 *   block output in the batch's format (ref: ...BaselineScanDecoder.cs:225-268 + the sink).
 * With JPGPU_OVERLAP=1 large batches (>= 4 Mi blocks of restart-interval scans) are issued as two halves of images on two
 * streams, the Huffman stage of the second half beside the output stage of the first; the first call after an upload or a
 * jpgpu_batch_stage_ms query and every 8th after it still run serially so that stage times exist.  Off by default: it
 * stopped paying once both stages became HBM-heavy.  Results do not depend on the issue order. */
int jpgpu_batch_decode(jpgpu_batch *b);
/* A progressive (SOF2) file that FAILS still leaves what the reference leaves in the writer's buffer: Decode()'s finally disposes the
 * scan decoder, which transforms and flushes the partial store (JpegDecoder.cs:545-549).  jpgpu_batch_result reports the failure,
 * jpgpu_batch_download_output of that image returns the partial picture (the step is issued a second time for such a batch, once
 * per upload; sequential files write nothing on failure that the reference would not). */
/* Individual stages, for stage-level parity tests and profiling. */
int jpgpu_batch_run_entropy(jpgpu_batch *b); /* marker index + Huffman -> coefficient buffer */
int jpgpu_batch_run_idct(jpgpu_batch *b);    /* coefficient buffer -> output */
/* RGB_PLANAR_F16 / _F32: the per-channel constants of the output stage (see the formats).  They belong to the batch, not to an upload: they
 * hold from the next jpgpu_batch_decode / jpgpu_batch_run_idct on, without a new upload, until they are set again.  A NULL pointer or a
 * constant that is not finite: JPGPU_ERR_ARGUMENT, and the constants in force stay.  The other formats never read them. */
int jpgpu_batch_set_output_affine(jpgpu_batch *b, const float scale[3], const float bias[3]);
/* The resize stage (K4).  While a resize is set, every jpgpu_batch_decode / jpgpu_batch_run_idct of a JPGPU_FMT_RGB_PLANAR_U8 upload is
 * followed, on the context's stream behind everything the output stage enqueues, by ONE launch that resamples every image (its window, if it
 * has one) to out_width x out_height and writes one dense buffer T[N][3][out_height][out_width] of sample_format's samples
 * (JPGPU_FMT_RGB_PLANAR_U8 / _F16 / _F32: uint8, binary16, float32).  The per-image outputs stay what they are.
 *
 * The result is a fixed function of the RGB_PLANAR_U8 bytes: separable antialiased bilinear resampling (a triangle filter, widened by the
 * scale when shrinking).  For an axis of input length I and output length O, in IEEE double:
 *     scale = I / O;  sup = max(scale, 1.0)
 *     for o in 0 .. O-1:
 *         c  = (o + 0.5) * scale
 *         lo = max(0, (int)(c - sup + 0.5));  hi = min(I, (int)(c + sup + 0.5))        ((int): truncation toward zero)
 *         w64[k] = max(0.0, 1.0 - fabs((k + lo - c + 0.5) / sup))   for k in 0 .. hi-lo-1
 *         w[k]   = (float)(w64[k] / sum(w64))                        (the sum in ascending k)
 * A horizontal pass, then a vertical pass, each  acc = 0.0f; for k ascending: t = w[k] * x; acc = acc + t  with every multiply and add
 * rounded to float32 on its own, never fused; x is (float)byte in the first pass and the first pass's float32 result in the second.  With v
 * the second pass's result the sample is  U8: clamp(rint(v), 0, 255), ties to even;  F32: (v * scale[c]) + bias[c] with the constants of
 * jpgpu_batch_set_output_affine, two roundings;  F16: that value rounded to nearest even to binary16.  At the image's own size every sample
 * is bit for bit what RGB_PLANAR_U8 / _F16 / _F32 hold.
 *
 * Like the constants, the setting is launch state of the batch: it holds from the next decode / run_idct until it is set again;
 * (0, 0, any format) withdraws it, and with it what an earlier decode left.  JPGPU_ERR_ARGUMENT, the setting in force kept, for a NULL
 * batch, a negative size, exactly one zero size, a size above 65535 or another format.  With a resize set, a decode / run_idct of an upload
 * whose format is not RGB_PLANAR_U8 returns JPGPU_ERR_ARGUMENT before anything is enqueued.  An image whose status is not 0 takes no part:
 * its slab reads as zeros.  Not resized: jpgpu_decoder_*, jpgpu_decode_scan, jpgpu_progressive_*, jpgpu_multi_*. */
int jpgpu_batch_set_resize(jpgpu_batch *b, int out_width, int out_height, int sample_format);
/* The resized buffer in device memory (256-byte aligned; image i at i * 3 * out_height * out_width samples), good until the next upload, decode
 * or withdrawal, and one image's slab copied to the host (waits for the batch's work).  JPGPU_ERR_INVALID_OPERATION when no decode with a
 * resize set has run on the upload. */
int jpgpu_batch_resized_device(const jpgpu_batch *b, void **ptr, uint64_t *bytes);
int jpgpu_batch_download_resized(jpgpu_batch *b, int i, void *dst, uint64_t bytes);
/* Device time of the last resize launch, from an event pair of its own (synchronises).  jpgpu_batch_stage_ms does not include it: the launch
 * lies behind the last stage event. */
int jpgpu_batch_resize_ms(jpgpu_batch *b, float *ms);
int jpgpu_batch_sync(jpgpu_batch *b);

int jpgpu_batch_size(const jpgpu_batch *b);
int jpgpu_batch_image_info(const jpgpu_batch *b, int i, jpgpu_image_info *info);
/* Valid after jpgpu_batch_sync. */
int jpgpu_batch_result(jpgpu_batch *b, int i, jpgpu_image_result *res);

/* Device pointers (HBM) of the whole-batch buffers; outputs stay resident for downstream GPU consumers.
 * Samples the reference would leave as the caller's buffer held them -- MCUs behind an early EOI
 * (JpegHuffmanBaselineScanDecoder.cs:144-150), components no scan writes, images without any scan -- read as zero here:
 * the batch owns the buffer, and zero is what a freshly allocated managed array holds.  (jpgpu_decode_scan, which
 * decodes over the caller's own samples, leaves them alone.) */
void *jpgpu_batch_output_device(const jpgpu_batch *b, uint64_t *total_bytes);
/* The coefficient pointer holds dense int16[blocks][64] at every image's coef_offset.  Scans the Huffman stage handed to the IDCT stage in
 * another form are expanded into a dense copy first: the call then waits for the batch's device work, allocates (on first use) a second
 * buffer of the coefficient store's size and copies the store into it, and the pointer is that copy's, good until the next entropy stage or
 * upload.  NULL if that wait, allocation or copy fails (jpgpu_last_error says why).  *total_blocks counts the buffer's blocks, padding
 * between images included.  (The handle is const for compatibility; the call may change the batch's buffers as described.) */
void *jpgpu_batch_coefficients_device(const jpgpu_batch *b, uint64_t *total_blocks);
/* Copies one image's output / coefficient blocks (int16[blocks][64], zig-zag order, MCU scan order) to the host.  (A progressive
 * frame whose Dispose() is taken literally -- component slots that do not cover every component once, the partial flush of a
 * failed file -- is transformed IN its store: behind the output stage its "coefficients" are samples; the pass runs once per
 * entropy stage, a second jpgpu_batch_run_idct / jpgpu_progressive_dispose flushes the same samples again.)
 * A multi-scan baseline image whose plan did not hold -- a middle scan leaves one byte unread in front of its terminating
 * marker, and the file is planned again and decoded on its own -- has its output and result from that re-plan after every
 * stage call; its coefficients are refused with JPGPU_ERR_NOT_SUPPORTED (the batch's store holds what the first plan's scans
 * made of the file). */
int jpgpu_batch_download_output(jpgpu_batch *b, int i, void *dst, size_t cap);
int jpgpu_batch_download_coefficients(jpgpu_batch *b, int i, int16_t *dst, size_t cap_blocks);
/* Overwrites one image's coefficient blocks from the host (IDCT-stage parity tests; config-5 style accumulate-then-IDCT). */
int jpgpu_batch_upload_coefficients(jpgpu_batch *b, int i, const int16_t *src, size_t nblocks);

/* hipEvent timings (ms) on the ctx stream over the jpgpu_batch_decode calls issued since the previous query (synchronises):
 * ms[0] marker index, ms[1] Huffman, ms[2] IDCT+output, averaged over the calls that ran serially (see jpgpu_batch_decode);
 * ms[3] whole pipeline, averaged over all calls. */
int jpgpu_batch_stage_ms(jpgpu_batch *b, float ms[4]);
/* Synchronisation rounds the self-synchronising DRI = 0 decoder needed in the most recent decode (0 = not used: also behind an upload
 * without DRI = 0 scans that follows one with them, and in front of an upload's first decode).  The rounds
 * are enqueued ahead and checked on the device (jpgpu_batch_decode does not wait for them): valid after jpgpu_batch_sync /
 * _result / _download_*. */
int jpgpu_batch_subseq_rounds(const jpgpu_batch *b);
/* The partial flush of FAILING progressive files (the reference's Decode() disposes the scan decoder in its `finally`, which
 * transforms and flushes the store as the failing scan left it, JpegDecoder.cs:545-549): on by default -- the first call that
 * needs a status or an output after a decode in which a progressive frame failed issues those frames once more, scan by scan
 * (the other images of the batch are not touched).  on = 0: callers that only want the statuses and the outputs of the images
 * that decoded leave it out (also: environment JPGPU_NO_PARTIAL_FLUSH); the failed frames' outputs are then unspecified. */
int jpgpu_batch_set_partial_flush(jpgpu_batch *b, int on);
/* Partial-flush replays issued for this batch so far (0: no progressive frame has failed, or the replay is switched off). */
int jpgpu_batch_progressive_replays(const jpgpu_batch *b);
/* Waits of this batch's jpgpu_batch_sync calls behind which a workgroup of the one-pass marker index (a workgroup per 16 KiB of
 * entropy data that finds the running sums of the data in front of it by looking back at what the workgroups there have published)
 * had run out of patience and counted the data in front of it itself.  Not expected to be anything but 0 -- the wait is bounded so
 * that nothing can hang -- and of no consequence for the results.  Valid after jpgpu_batch_sync. */
int jpgpu_batch_marker_fallbacks(const jpgpu_batch *b);
/* Times the enqueued rounds did not reach the fixed point (the synchronising call then issued the step again with the host
 * reading the counts between rounds, and the upload's later decodes stay that way).  Counted for the batch: an upload does not reset it.
 * Valid after jpgpu_batch_sync. */
int jpgpu_batch_subseq_fallbacks(const jpgpu_batch *b);
/* Times the single-launch progressive path gave up waiting inside the kernel (its scans follow each other's progress, which
 * relies on workgroups being dispatched in list order) and the step was re-issued scan level by scan level.  Counted per upload: every
 * upload starts at 0 (jpgpu_batch_progressive_replays, _marker_fallbacks and _subseq_fallbacks count for the batch).  Valid after
 * jpgpu_batch_result. */
int jpgpu_batch_progressive_fallbacks(const jpgpu_batch *b);
/* How the last upload planned the scans of its progressive (SOF2) frames, and which launches the last decode / run_entropy
 * took for them (read only; for tests and tools).  A scan waits for the earlier scans of its frame that touch the same
 * coefficients: `levels` counts the launch groups that ordering gives, `max_deps` the most DIRECT producers any scan has
 * (more than three: the batch is not pipelined).  Chains: 0 = DC scans, 1 + min(3, c) = AC scans of frame component c. */
#define JPGPU_PROGRESSIVE_CHAINS 5
#define JPGPU_PROG_LAUNCH_NONE 0             /* no progressive scan was launched (yet) */
#define JPGPU_PROG_LAUNCH_PIPELINED_GATED 1  /* one launch, every workgroup resident, followers watch their producers */
#define JPGPU_PROG_LAUNCH_PIPELINED_FORCED 2 /* the same launch without the residency gate (JPGPU_PROG_FORCE_PIPELINE) */
#define JPGPU_PROG_LAUNCH_CHAINS 3           /* one stream per chain, one launch per scan ordinal of the chain */
#define JPGPU_PROG_LAUNCH_BY_LEVEL 4         /* one launch (pair) per dependency level */
typedef struct jpgpu_progressive_plan {
    int32_t scans;          /* progressive scans planned, over all frames */
    int32_t levels;         /* launch groups (dependency levels; scans in file order where the plan is scan by scan) */
    int32_t max_deps;       /* largest number of direct producers of one scan */
    int32_t pipelined;      /* the plan allows the single pipelined launch (0 after a fallback as well) */
    int32_t chains_ok;      /* the plan allows the chain launches */
    int32_t pipe_waves;     /* entries of the pipelined launch's list: one per wave */
    int32_t wave_tails;     /* scans that run behind their only producer in that producer's wave */
    int32_t lane_work;      /* work entries of the lane-per-interval kernel (scans of many restart intervals, empty bands) */
    int32_t chain_scans[JPGPU_PROGRESSIVE_CHAINS]; /* scans per chain */
    int32_t launch_form;    /* JPGPU_PROG_LAUNCH_* of the last decode / run_entropy */
} jpgpu_progressive_plan;
size_t jpgpu_sizeof_progressive_plan(void);
int jpgpu_batch_progressive_plan(const jpgpu_batch *b, jpgpu_progressive_plan *plan);
/* Total entropy-segment bytes / blocks / pixels of the successfully parsed images. */
int jpgpu_batch_totals(const jpgpu_batch *b, uint64_t *compressed_bytes, uint64_t *blocks, uint64_t *pixels,
                       uint64_t *output_bytes);

/* ------------------------------------------------------------------------------------------------ (1b) several devices
 * The multi-GPU driver of SURVEY.md 7 step 6 / 8e inside the library: one context, one batch and one host thread per listed
 * device, image i of a call on device slot i mod G (jpgpu_shard's rule), no exchange between the devices.  Replaces the
 * caller-side loop "one JpegDecoder per thread" (Threading) for a whole file list.  A device may be listed more than
 * once (two independent contexts on it).  jpgpu_multi_decode uploads and decodes every shard concurrently and returns when
 * all of them are done; results and outputs are then read through the shard's batch (jpgpu_batch_result,
 * jpgpu_batch_output_device / _download_output, ...) at the local index jpgpu_multi_locate gives. */
typedef struct jpgpu_multi jpgpu_multi;
int jpgpu_multi_create(const int *devices, int n_devices, jpgpu_multi **out);
void jpgpu_multi_destroy(jpgpu_multi *m);
int jpgpu_multi_devices(const jpgpu_multi *m);
const char *jpgpu_multi_last_error(const jpgpu_multi *m);
/* Decodes n files in `format`; returns the first non-OK call status of any shard (per-image failures are per-image results, as
 * with jpgpu_batch_*).  upload_ms / decode_ms (may be NULL): the slowest shard's time in each phase. */
int jpgpu_multi_decode(jpgpu_multi *m, const uint8_t *const *jpeg, const size_t *len, int n, int format, double *upload_ms,
                       double *decode_ms);
/* The same in two halves, for callers that feed the devices continuously.  Every slot owns TWO batches: jpgpu_multi_submit
 * uploads call k's shards into the idle one of each slot, launches their decode and returns while the devices work;
 * jpgpu_multi_wait(ticket) blocks until that call's decodes are done.  Submitting call k+1 before waiting for call k puts its
 * host parse + H2D beside call k's decode (upload stream / decode stream of each context); at most two calls may be in
 * flight, and a ticket's outputs stay valid until the second submit after it.  flags: JPGPU_UPLOAD_PINNED as in
 * jpgpu_batch_upload_segments (every file one page-locked segment).  The host crew of slot s is (CPUs granted to the
 * process) / G threads -- G slots share the machine -- unless jpgpu_set_host_threads / JPGPU_HOST_THREADS says otherwise.
 * A submit that fails (any slot's upload or launch) takes no ticket (*ticket = -1): the slots that did launch are waited
 * for before it returns, nothing stays in flight and the next submit may use the same batches. */
int jpgpu_multi_submit(jpgpu_multi *m, const uint8_t *const *jpeg, const size_t *len, int n, int format, unsigned flags, int *ticket);
int jpgpu_multi_wait(jpgpu_multi *m, int ticket, double *upload_ms, double *decode_ms);
jpgpu_batch *jpgpu_multi_batch_of(jpgpu_multi *m, int ticket, int slot);
/* Where image i of the last jpgpu_multi_decode went: the device slot (index into `devices`) and its index in that slot's batch. */
int jpgpu_multi_locate(const jpgpu_multi *m, int i, int *slot, int *local_index);
jpgpu_batch *jpgpu_multi_batch(jpgpu_multi *m, int slot); /* of the most recent jpgpu_multi_decode / _submit */
jpgpu_ctx *jpgpu_multi_context(jpgpu_multi *m, int slot);

/* ------------------------------------------------------------------------------------------------ (2) per scan
 * Replaces JpegScanDecoder.ProcessScan(ref JpegReader, JpegScanHeader) for SOF0/SOF1
 * (ref: ScanDecoder/JpegScanDecoder.cs:12-36, ScanDecoder/JpegHuffmanBaselineScanDecoder.cs:51-177).
 * The scan decoder's pulled inputs become arguments: GetRestartInterval (JpegDecoder.cs:656),
 * GetHuffmanTable (:869), GetQuantizationTable (:910).  qt is in zig-zag order like
 * JpegQuantizationTable.Elements (JpegQuantizationTable.cs:47); qt_present[i] = !IsEmpty.
 * dht[0][id] are DC tables, dht[1][id] AC tables.  `entropy` points just after the SOS segment
 * (reader.RemainingBytes); *bytes_consumed is what the reference advances the reader by.
 * Output is written to host memory `out` (cap bytes) in `format`; what `out` holds on entry is the canvas: samples the
 * scan does not write (other components of a non-interleaved scan, MCUs behind an early EOI) keep their values, as
 * with the reference's writers (JpegBufferOutputWriter8Bit.cs:28-60).
 */
int jpgpu_decode_scan(jpgpu_ctx *ctx, const jpgpu_frame *frame, const jpgpu_scan *scan, const uint16_t qt[4][64],
                      const uint8_t qt_present[4], const jpgpu_dht dht[2][4], uint16_t restart_interval,
                      const uint8_t *entropy, size_t len, int format, void *out, size_t cap,
                      jpgpu_image_result *result, size_t *bytes_consumed);

/* ------------------------------------------------------------------------------------------------ (2b) per scan, SOF2
 * Replaces JpegHuffmanProgressiveScanDecoder behind JpegScanDecoder.Create(SOF2, ...) (ScanDecoder/JpegScanDecoder.cs:18-36):
 * what JpegDecoder.ProcessFrameHeader / ProcessScanHeader / Decode's finally call on it (JpegDecoder.cs:562-570, 592-599,
 * 545-549), so that a C# JpegDecoder keeps its own marker loop for progressive files too.
 *   jpgpu_progressive_begin    the constructor (ScanDecoder/JpegHuffmanProgressiveScanDecoder.cs:23-55): MCU geometry, and
 *                              JpegBlockAllocator.Allocate (JpegBlockAllocator.cs:35-84) -- the zeroed coefficient store, in HBM,
 *                              where it stays between the calls.
 *   jpgpu_progressive_scan     ProcessScan (:57-90): resolves the scan's components against the tables passed (the decoder's
 *                              registry at this SOS: GetHuffmanTable / GetQuantizationTable, JpegDecoder.cs:869, 910) and the
 *                              restart interval in force NOW (GetRestartInterval read per scan, :78 -- it may change between
 *                              scans), then decodes the scan into the store on the GPU before it returns: the status is this
 *                              scan's (reference exception classes and messages, as jpgpu_decode_scan).  `entropy` = the bytes
 *                              behind the SOS header; the segment ends at the first marker that is not RSTn.  *bytes_consumed is
 *                              always 0: the reference's progressive ProcessScan never advances the outer reader, Decode's
 *                              TryReadMarker finds the next marker by itself (JpegReader.cs:120-158).
 *   jpgpu_progressive_dispose  Dispose (:421-470): dequantise + IDCT + level shift over the MCU grid with the quantisation tables
 *                              the LAST scans left in the decoder's component slots, then
 *                              JpegBlockAllocator.Flush (JpegBlockAllocator.cs:120-190) into `out` in `format`
 *                              (jpgpu_progressive_output_size says how large), or, _to_writer, as WriteBlock calls in Flush's order.
 *                              Scan orders whose slots do not cover every component once are disposed the way the reference does it
 *                              (a component transformed twice, another never: dispose_pass_kernel); a session without any scan
 *                              flushes the zeroed store.  After a FAILING jpgpu_progressive_scan the store holds what the
 *                              reference's ProcessScan left when it threw -- every coefficient and correction bit in front of the
 *                              throw, nothing behind it: the failing scan is issued once more from a device copy of the store taken
 *                              in front of it, coefficient by coefficient up to the failing restart interval -- so a dispose behind
 *                              it flushes what Decode()'s `finally` flushes (JpegDecoder.cs:545-549), like the batch entry points.
 */
typedef struct jpgpu_progressive jpgpu_progressive;
int jpgpu_progressive_begin(jpgpu_ctx *ctx, const jpgpu_frame *frame, jpgpu_progressive **out);
int jpgpu_progressive_scan(jpgpu_progressive *p, const jpgpu_scan *scan, const uint16_t qt[4][64], const uint8_t qt_present[4],
                           const jpgpu_dht dht[2][4], uint16_t restart_interval, const uint8_t *entropy, size_t len,
                           jpgpu_image_result *result, size_t *bytes_consumed);
int jpgpu_progressive_output_size(jpgpu_progressive *p, int format, size_t *bytes);
int jpgpu_progressive_dispose(jpgpu_progressive *p, int format, void *out, size_t cap);
void jpgpu_progressive_destroy(jpgpu_progressive *p);

/* ------------------------------------------------------------------------------------------------ (3) decoder
 * Handle-based mirror of the public JpegDecoder surface (ref: JpegDecoder.cs).  Names follow the reference.
 */
/* ref: JpegBlockOutputWriter.WriteBlock (JpegBlockOutputWriter.cs:17): 64 int16 row-major, unclamped,
 * full-resolution pixel coordinates; same call order as the reference (MCU raster, scan-component order,
 * block raster in MCU, sub-block raster for expanded chroma). */
typedef void (*jpgpu_write_block_fn)(void *user, const int16_t *block, int component_index, int x, int y);

/* jpgpu_progressive_dispose for an arbitrary JpegBlockOutputWriter: the IDCT pass on the GPU, then the WriteBlock calls of
 * JpegBlockAllocator.Flush (component, block row, block column; sub-sampled components expanded) replayed on the host. */
int jpgpu_progressive_dispose_to_writer(jpgpu_progressive *p, jpgpu_write_block_fn fn, void *user);

/* ctx may be NULL for host-only use (Identify / metadata / tables); Decode then returns JPGPU_ERR_NO_DEVICE. */
int jpgpu_decoder_create(jpgpu_ctx *ctx, jpgpu_decoder **out);          /* new JpegDecoder()                */
void jpgpu_decoder_destroy(jpgpu_decoder *d);
const char *jpgpu_decoder_last_error(const jpgpu_decoder *d);
int jpgpu_decoder_set_input(jpgpu_decoder *d, const uint8_t *data, size_t len); /* SetInput  :49-62    */
int jpgpu_decoder_identify(jpgpu_decoder *d, int load_quantization_tables, int *stream_length); /* Identify :75-105 */
int jpgpu_decoder_try_estimate_quality(jpgpu_decoder *d, float *quality);       /* TryEstimateQuanlity :169-196 */
int jpgpu_decoder_width(const jpgpu_decoder *d);                                 /* Width  :383 (-1: no frame header) */
int jpgpu_decoder_height(const jpgpu_decoder *d);                                /* Height :388 */
int jpgpu_decoder_precision(const jpgpu_decoder *d);                             /* Precision :393 */
int jpgpu_decoder_number_of_components(const jpgpu_decoder *d);                  /* NumberOfComponents :398 */
int jpgpu_decoder_start_of_frame(const jpgpu_decoder *d);                        /* StartOfFrame :43 */
int jpgpu_decoder_get_maximum_horizontal_sampling(jpgpu_decoder *d);             /* :413 */
int jpgpu_decoder_get_maximum_vertical_sampling(jpgpu_decoder *d);               /* :436 */
int jpgpu_decoder_get_horizontal_sampling(jpgpu_decoder *d, int component_index); /* :462 */
int jpgpu_decoder_get_vertical_sampling(jpgpu_decoder *d, int component_index);   /* :481 */
int jpgpu_decoder_get_restart_interval(const jpgpu_decoder *d);                  /* GetRestartInterval :656 */
int jpgpu_decoder_set_restart_interval(jpgpu_decoder *d, int restart_interval);  /* SetRestartInterval :662 */
int jpgpu_decoder_load_tables(jpgpu_decoder *d, const uint8_t *data, size_t len); /* LoadTables :313-363 */
/* SetOutputWriter :501 -- generic writer: blocks are decoded on the GPU (PLANAR_I16) and replayed on the host. */
int jpgpu_decoder_set_output_writer(jpgpu_decoder *d, jpgpu_write_block_fn fn, void *user);
/* SetOutputWriter with the reference's stock 8-bit sink (apps/JpegDecode/JpegBufferOutputWriter8Bit.cs):
 * the interleaved buffer is produced directly on the GPU (INTERLEAVED_U8) and copied into `out`. */
int jpgpu_decoder_set_output_buffer8(jpgpu_decoder *d, int width, int height, int component_count, uint8_t *out,
                                     size_t cap);
/* SetOutputWriter with the reference's other two stock sinks (apps/JpegDecode/JpegBufferOutputWriterLessThan8Bit.cs,
 * JpegBufferOutputWriterGreaterThan8Bit.cs; the writer's own `precision`, 1..16, picks the conversion, 8 is the 8-bit sink's):
 * produced directly on the GPU (INTERLEAVED_U8_SCALED) when width, height, component count and precision equal the frame's,
 * else the writer is replayed on the host with its own precision. */
int jpgpu_decoder_set_output_buffer8_scaled(jpgpu_decoder *d, int width, int height, int precision, int component_count, uint8_t *out,
                                            size_t cap);
int jpgpu_decoder_decode(jpgpu_decoder *d);                                      /* Decode :509-550 */
/* The TIFF-style surface (JPEG-in-TIFF keeps tables, frame header and strips apart; SURVEY 5 "checkpoint / resume" row): the
 * caller sets the pieces itself instead of letting Decode()'s marker loop find them, then hands over one scan's entropy data. */
int jpgpu_decoder_set_start_of_frame(jpgpu_decoder *d, int marker);              /* StartOfFrame { set; } :43 (0xC0 / 0xC1 / 0xC2) */
int jpgpu_decoder_set_frame_header(jpgpu_decoder *d, const jpgpu_frame *frame);  /* SetFrameHeader :404-407 (frame->sof is NOT applied) */
/* SetHuffmanTable(JpegHuffmanDecodingTable) :793-815: replaces the entry with the same class (0 = DC, 1 = AC) and identifier */
int jpgpu_decoder_set_huffman_table(jpgpu_decoder *d, int table_class, int identifier, const uint8_t bits[16], const uint8_t *values,
                                    int num_values);
/* SetQuantizationTable(JpegQuantizationTable) :840-861: 64 elements in zig-zag order (JpegQuantizationTable.cs:47) */
int jpgpu_decoder_set_quantization_table(jpgpu_decoder *d, int element_precision, int identifier, const uint16_t *zigzag64);
int jpgpu_decoder_clear_huffman_table(jpgpu_decoder *d);                         /* ClearHuffmanTable :768-771 */
int jpgpu_decoder_clear_quantization_table(jpgpu_decoder *d);                    /* ClearQuantizationTable :784-787 */
/* ProcessScan(ref JpegReader, JpegScanHeader) :624-632: JpegScanDecoder.Create(StartOfFrame, this, GetFrameHeader()) -- the restart
 * interval is latched at this moment -- one ProcessScan over `entropy` (reader.RemainingBytes), Dispose.  The output
 * goes to the writer set with jpgpu_decoder_set_output_writer / _set_output_buffer8 / _set_output_buffer8_scaled; *bytes_consumed = the reader's advance. */
int jpgpu_decoder_process_scan(jpgpu_decoder *d, const jpgpu_scan *scan, const uint8_t *entropy, size_t len, size_t *bytes_consumed);
void jpgpu_decoder_reset(jpgpu_decoder *d);                                      /* Reset :930 */
void jpgpu_decoder_reset_input(jpgpu_decoder *d);                                /* ResetInput :941 */
void jpgpu_decoder_reset_header(jpgpu_decoder *d);                               /* ResetHeader :949 */
void jpgpu_decoder_reset_tables(jpgpu_decoder *d);                               /* ResetTables :960 */
void jpgpu_decoder_reset_output_writer(jpgpu_decoder *d);                        /* ResetOutputWriter :975 */

/* ------------------------------------------------------------------------------------------------ (4) encoder
 * The step on the other side of the wire format: JpegEncoder.Encode() (ref: JpegEncoder.cs:255-291)
 * for a batch of images, with the call sequence of apps/JpegEncode/EncodeAction.cs:38-63 (optimizeCoding = false):
 *   SetQuantizationTable(ScaleByQuality(luminance, 0, quality)), SetQuantizationTable(ScaleByQuality(chrominance, 1, quality)),
 *   SetHuffmanTable(DC/AC, 0/1, standard tables), AddComponent(1, 0, 0, 0, luma_h, luma_v) [, AddComponent(2 | 3, 1, 1, 1, 1, 1)],
 *   SetInputReader(JpegBufferInputReader(width, height, components, pixels)), Encode().
 * The output is the byte stream the reference writes (SOI, DQT, SOF0, DHT, SOS, entropy data, EOI).
 * input_rgb == 1: pixels are R,G,B and JpegRgbToYCbCrConverter.ConvertRgb24ToYCbCr8 (apps/JpegEncode/
 * JpegRgbToYCbCrConverter.cs:64-96) is applied first, like EncodeAction.cs:31-36 does.  input_rgb == 2: pixels are Rgba32
 * (four bytes each, the alpha byte stepped over) and ConvertRgba32ToYCbCr8 is applied, like the reference's EncoderBenchmark does
 * (tests/JpegLibrary.Benchmarks/EncoderBenchmark.cs:93, ColorConverters/JpegRgbToYCbCrConverter.cs:95-124): same tables. */
typedef struct jpgpu_encode_params {
    int32_t width, height;
    int32_t components;      /* encoded components: 1 or 3 == samples per pixel of the input buffer (input_rgb == 2: four bytes per pixel) */
    int32_t luma_h, luma_v;  /* sampling factors of the first component (1, 2 or 4); the others are 1 x 1 */
    int32_t quality;         /* 1..100, JpegStandardQuantizationTable.ScaleByQuality */
    int32_t input_rgb;       /* 0, 1 or 2, see above */
    int32_t optimize_coding; /* 1 = EncodeAction's optimizeCoding (EncodeAction.cs:40-46): Huffman tables built from the image's own
                                statistics (TransformBlocks / BuildHuffmanTables / WritePreparedScanData, JpegEncoder.cs:264-274);
                                2 = the same with JpegEncoder.MostOptimalCoding (:43) */
    int32_t restart_interval; /* 0 = none = everything the reference's encoder can write.  n > 0 is an EXTENSION (SURVEY.md 8f N3,
                                "+ DRI emission"; JpegEncoder has no restart support): a DRI segment in front of SOF0 and, in front
                                of every MCU whose index is a non-zero multiple of n, one-bit padding to a byte boundary, RSTm
                                (m modulo 8) and the DC predictors back at zero (T.81 B.2.4.4 / E.1.4: what libjpeg writes, and what
                                JpegDecoder reads back: ScanDecoder/JpegHuffmanBaselineScanDecoder.cs:139-163).  1..65535 */
} jpgpu_encode_params;
typedef struct jpgpu_encoder jpgpu_encoder;

int jpgpu_encoder_create(jpgpu_ctx *ctx, jpgpu_encoder **out);
void jpgpu_encoder_destroy(jpgpu_encoder *e);
/* SetInputReader for n images (host parse of nothing: pixels go to HBM as they are) */
int jpgpu_encoder_upload(jpgpu_encoder *e, const uint8_t *const *pixels, const jpgpu_encode_params *params, int n);
/* SetQuantizationTable(new JpegQuantizationTable(0, identifier, elements)) for image i (JpegEncoder.cs:102-126): the caller's own
 * table instead of the standard one scaled by `quality`.  identifier 0 = the first component's table, 1 = the other components';
 * 64 elements in zig-zag order, element precision 0, so 1..255 each (the segment stores bytes; 0 would divide by zero in
 * ZigZagAndQuantizeBlock).  Between jpgpu_encoder_upload and jpgpu_encoder_encode.  Behind jpgpu_encoder_upload_described it is
 * JPGPU_ERR_INVALID_OPERATION for every image: a description carries its tables. */
int jpgpu_encoder_set_quantization_table(jpgpu_encoder *e, int i, int identifier, const uint16_t *zigzag64);
/* Encode(): FDCT + quantise, Huffman code lengths, bit emission, byte stuffing -- all on the device */
int jpgpu_encoder_encode(jpgpu_encoder *e);
/* Device time (ms, HIP events) of the last jpgpu_encoder_encode by stage: ms[0] pixels -> quantised zig-zag blocks (ReadBlock, FDCT,
 * ZigZagAndQuantizeBlock: JpegEncoder.cs:662-741, 812-826; with optimize_coding also GatherBlockStatistics :552-597), ms[1] code lengths
 * and bit offsets, ms[2] bit emission (EncodeBlock :828-925), ms[3] byte stuffing (JpegWriter.cs:133-232), ms[4] their sum.  Which kernels
 * of JPGPU_CODING_OPTIMIZED and JPGPU_CODING_PROGRESSIVE count in which entry: (4e), "Stages". */
int jpgpu_encoder_stage_ms(jpgpu_encoder *e, float ms[5]);
/* How the entropy stage of this encoder's jpgpu_encoder_encode calls ran: *one_pass = calls that counted and emitted the bits in ONE
 * pass over the blocks (uploads of two or more images without restart intervals: EncodeBlock, JpegEncoder.cs:828-925, run once per
 * block instead of twice), *fell_back = those of them that had to issue the two-kernel form behind it (a workgroup's stretch of the
 * stream beyond the on-chip buffer: noise at quality 100).  The streams are the same bytes either way.  Either pointer may be NULL. */
int jpgpu_encoder_emit_passes(const jpgpu_encoder *e, int *one_pass, int *fell_back);
int jpgpu_encoder_encoded_size(const jpgpu_encoder *e, int i, size_t *bytes);
int jpgpu_encoder_download(jpgpu_encoder *e, int i, void *dst, size_t cap);                       /* the IBufferWriter's content */
void *jpgpu_encoder_output_device(const jpgpu_encoder *e, int i, size_t *bytes);                  /* stream i, resident in HBM */
/* quantised zig-zag blocks in encoding order (what ZigZagAndQuantizeBlock produced, JpegEncoder.cs:812-826) */
int jpgpu_encoder_download_coefficients(jpgpu_encoder *e, int i, int16_t *dst, size_t cap_blocks);

/* ---- (4b) described images: every component arrangement JpegEncoder.AddComponent accepts (JpegEncoder.cs:175-240).
 * A jpgpu_encode_description is the encoder's state after the caller's Set* / AddComponent sequence, list by list:
 *   components      AddComponent order.  A component reads sample number (position in this list) of every input pixel
 *                   (component.Index, JpegBufferInputReader.cs:47), whatever its component_index says.
 *   quant_tables    SetQuantizationTable order: the stream's DQT, written whole (WriteQuantizationTables :305-330) and independent
 *                   of what the components captured (a table replaced after AddComponent reaches the DQT, not the component).
 *   huffman_tables  SetHuffmanTable order: the stream's DHT.  given = 1: a JpegHuffmanEncodingTable(JpegHuffmanCanonicalCode[])
 *                   as the caller built it -- TryWrite (JpegHuffmanEncodingTable.cs:50-86) decides the DHT bytes, GetCode
 *                   (:94-100) the code of all 256 symbols (a symbol the table does not hold gets entry 0's code and length);
 *                   given = 0: left to be built from the image (JpegHuffmanEncodingTableBuilder).
 * Any table to be built sends the image down TransformBlocks / BuildHuffmanTables / WritePreparedScanData (:264-274), none down
 * WriteScanData (:278-280).  A builder no component feeds makes Build throw "No symbol is recorded.": the image's status
 * (JPGPU_ERR_INVALID_OPERATION), as with jpgpu_encoder_upload.  An arrangement without a component at the maximum sampling factors
 * in both directions (2 x 1 beside 1 x 2) is refused: JPGPU_ERR_NOT_SUPPORTED as that image's status, see DESIGN.md section 5.
 * An EncodeAction arrangement (what jpgpu_encoder_upload describes) gives the bytes jpgpu_encoder_upload gives. */
#define JPGPU_ENC_MAX_COMPONENTS 4
#define JPGPU_ENC_MAX_TABLES 8
typedef struct jpgpu_encode_component {
    uint8_t component_index;  /* the identifier SOF0 and SOS carry */
    uint8_t h, v;             /* sampling factors: 1, 2 or 4 */
    uint8_t tq;               /* identifier of the captured quantisation table (written to SOF0) */
    uint8_t td, ta;           /* DC / AC Huffman table identifiers (looked up in huffman_tables, first match) */
    uint8_t reserved[2];
    uint16_t quant[64];       /* the 64 elements AddComponent captured, zig-zag order, 1..255 */
} jpgpu_encode_component;
typedef struct jpgpu_encode_quant_table {
    uint8_t identifier;
    uint8_t reserved;
    uint16_t elements[64];    /* zig-zag order, 1..255 */
} jpgpu_encode_quant_table;
typedef struct jpgpu_encode_huffman_table {
    uint8_t table_class;      /* 0 = DC, 1 = AC */
    uint8_t identifier;       /* identifier & 0xf goes into the Tc/Th byte */
    uint8_t given;            /* 1: the codes below; 0: built from the image */
    uint8_t reserved;
    int32_t num_codes;        /* given: 1..256 entries of the JpegHuffmanCanonicalCode[] */
    uint16_t code[256];       /* .Code (below 2^length) */
    uint8_t symbol[256];      /* .Symbol */
    uint8_t length[256];      /* .CodeLength, 0..16 (0 = an entry TryWrite leaves out; such entries come first) */
} jpgpu_encode_huffman_table;
typedef struct jpgpu_encode_description {
    int32_t width, height;
    int32_t in_components;       /* samples per input pixel, at least num_components */
    int32_t input_rgb;           /* 0; 1 (R,G,B) or 2 (R,G,B,A) with exactly three components, as in jpgpu_encode_params */
    int32_t restart_interval;    /* the extension of jpgpu_encode_params */
    int32_t most_optimal_coding; /* JpegEncoder.MostOptimalCoding */
    int32_t num_components, num_quant_tables, num_huffman_tables;
    int32_t reserved;
    jpgpu_encode_component components[JPGPU_ENC_MAX_COMPONENTS];
    jpgpu_encode_quant_table quant_tables[JPGPU_ENC_MAX_TABLES];
    jpgpu_encode_huffman_table huffman_tables[JPGPU_ENC_MAX_TABLES];
} jpgpu_encode_description;
size_t jpgpu_sizeof_encode_component(void);
size_t jpgpu_sizeof_encode_quant_table(void);
size_t jpgpu_sizeof_encode_huffman_table(void);
size_t jpgpu_sizeof_encode_description(void);
/* jpgpu_encoder_upload for described images.  Argument errors fail the call; a refused arrangement is that image's status alone.
 * An upload that holds an image the general kernels take counts and emits the bits of ALL its images as two kernels
 * (jpgpu_encoder_emit_passes: no one-pass call); uploads of EncodeAction arrangements alone run as they always did. */
int jpgpu_encoder_upload_described(jpgpu_encoder *e, const uint8_t *const *pixels, const jpgpu_encode_description *desc, int n);
/* ---- (4c) pixels that are on the device already: jpgpu_encoder_upload / jpgpu_encoder_upload_described without the copy.
 * device_pixels[i] is device memory of the context's device that holds image i's pixels; pixel_layouts[i] says how (NULL: all
 * JPGPU_PIXELS_INTERLEAVED):
 *   JPGPU_PIXELS_INTERLEAVED  (height, width, in_components) -- what the host entries take (in_components: 4 with input_rgb == 2)
 *   JPGPU_PIXELS_PLANAR       in_components tight planes of height x width bytes: sample c of pixel (x, y) is byte
 *                             c * height * width + y * width + x (a torch uint8[C, H, W] tensor, FMT RGB_PLANAR_U8's output)
 * Rows and planes are tight: no pitch.  Any address will do; images whose address, row length (and plane size) are multiples of
 * 16 bytes take the widest loads.  An upload is all-host or all-device.  Everything behind the upload
 * (jpgpu_encoder_set_quantization_table, _encode, _stage_ms, _emit_passes, _download, _download_coefficients, _image_status)
 * behaves as it does behind a host upload, and the streams are the same bytes.
 * NOTHING IS COPIED: jpgpu_encoder_encode reads the caller's memory.  It must stay valid and unwritten from this call until
 * jpgpu_encoder_encode returns (which ends with a synchronisation of the context's stream), for every encode of this upload; and
 * the work that produced the pixels must be complete -- or ordered before the context's stream -- when this call is made.
 * JPGPU_ERR_ARGUMENT for the whole call, decided here and before anything is enqueued: a NULL encoder, array or pixel pointer; a
 * pointer hipPointerGetAttributes does not report as device memory of the context's device (host, pinned host and managed memory
 * are refused); an image whose width * height * in_components bytes do not lie inside ONE allocation (hipMemGetAddressRange); a
 * layout other than the two above; input_rgb == 2 with JPGPU_PIXELS_PLANAR (no alpha plane is defined).  A refused upload leaves
 * the encoder empty. */
#define JPGPU_PIXELS_INTERLEAVED 0
#define JPGPU_PIXELS_PLANAR 1
int jpgpu_encoder_upload_device(jpgpu_encoder *e, const void *const *device_pixels, const jpgpu_encode_params *params,
                                const int32_t *pixel_layouts, int n);
int jpgpu_encoder_upload_described_device(jpgpu_encoder *e, const void *const *device_pixels, const jpgpu_encode_description *desc,
                                          const int32_t *pixel_layouts, int n);
/* ---- (4d) Arithmetic: the file libjpeg writes in place of the reference's (an extension beyond the reference; what Pillow's
 * Image.save(f, "JPEG", quality=q, subsampling=s), torchvision.io.encode_jpeg and OpenCV write, all on libjpeg-turbo's jpeg_fdct_islow).
 *   By default (JPGPU_ARITHMETIC_REFERENCE) every stream is what it was, byte for byte.  Under JPGPU_ARITHMETIC_LIBJPEG the stream of an
 * image of jpgpu_encoder_upload / jpgpu_encoder_upload_device is, from SOI to EOI, the file libjpeg's baseline compressor writes for the
 * same pixels, quality and sampling with its default settings (Annex K Huffman tables, no optimisation, no smoothing).  Per image:
 *   1. TABLES.  s = quality < 50 ? 5000 / quality : 200 - 2 * quality; element = clamp((std * s + 50) / 100, 1, 255) over the Annex K
 *     luminance (table 0) and chrominance (table 1) tables, integer division.  jpgpu_encoder_set_quantization_table replaces one.
 *   2. COLOUR, input_rgb 1 and 2 (2: the alpha byte stepped over):
 *       Y = (19595 R + 38470 G + 7471 B + 32768) >> 16          Cb = (-11059 R - 21709 G + 32768 B + (128 << 16) + 32767) >> 16
 *       Cr = (32768 R - 27439 G - 5329 B + (128 << 16) + 32767) >> 16
 *     input_rgb == 0 with three components takes the samples as they are (Pillow's mode "YCbCr").
 *   3. GEOMETRY AND EDGES.  Three components: luma (H, V) = (luma_h, luma_v), one of 1 x 1, 2 x 1, 2 x 2; chroma 1 x 1; an interleaved scan
 *     of ceil(W / 8H) x ceil(Ht / 8V) MCUs.  A component with factors (h, v) has wb = ceil(ceil(W h / H) / 8) by hb = ceil(ceil(Ht v / V) / 8)
 *     blocks of its own.  The last pixel column of the full-size plane is repeated out to wb * 8 * (H / h) columns, the last pixel row out
 *     to a multiple of V rows and no further; then the plane is downsampled -- H / h = V / v = 2: (a + b + c + d + bias) >> 2 with bias 1, 2,
 *     1, 2, ... along the output row; H / h = 2 alone: (a + b + bias) >> 1 with bias 0, 1, 0, 1, ...; else a copy -- and the last DOWNSAMPLED
 *     row is repeated out to hb * 8 rows.  One component: a non-interleaved scan of ceil(W / 8) x ceil(Ht / 8) MCUs of one block, whatever
 *     luma_h and luma_v say (they must be one of the three shapes); SOF0 carries 1 x 1, as Pillow writes it.
 *   4. DUMMY BLOCKS.  A block of an MCU at bx >= wb or by >= hb of its component is not transformed: its AC values are zero, its DC is the
 *     quantised DC of the block emitted just before it in the same MCU (the first block of a component in an MCU always lies inside).
 *   5. THE TRANSFORM, jfdctint.c with CONST_BITS = 13, PASS1_BITS = 2, on sample - 128, the eight values d0..d7 of each ROW first, then
 *     of each COLUMN of what the rows left, DESCALE(x, n) = (x + (1 << (n - 1))) >> n an arithmetic shift:
 *       t0 = d0 + d7   t1 = d1 + d6   t2 = d2 + d5   t3 = d3 + d4       t7 = d0 - d7   t6 = d1 - d6   t5 = d2 - d5   t4 = d3 - d4
 *       t10 = t0 + t3   t13 = t0 - t3   t11 = t1 + t2   t12 = t1 - t2
 *       rows: o0 = (t10 + t11) << 2, o4 = (t10 - t11) << 2, n = 11     columns: o0 = DESCALE(t10 + t11, 2), o4 = DESCALE(t10 - t11, 2), n = 15
 *       z1 = (t12 + t13) * 4433      o2 = DESCALE(z1 + t13 * 6270, n)      o6 = DESCALE(z1 - t12 * 15137, n)
 *       z1 = t4 + t7   z2 = t5 + t6   z3 = t4 + t6   z4 = t5 + t7   z5 = (z3 + z4) * 9633
 *       t4 *= 2446   t5 *= 16819   t6 *= 25172   t7 *= 12299   z1 *= -7373   z2 *= -20995   z3 = z3 * -16069 + z5   z4 = z4 * -3196 + z5
 *       o7 = DESCALE(t4 + z1 + z3, n)   o5 = DESCALE(t5 + z2 + z4, n)   o3 = DESCALE(t6 + z2 + z3, n)   o1 = DESCALE(t7 + z1 + z4, n)
 *     All in 32-bit integers, which 8-bit samples never leave.  The result is 8 times the DCT.
 *   6. QUANTISATION.  d = Q << 3, m = (|c| + (d >> 1)) / d, integer division; the value is -m where c < 0 (halves round away from zero).
 *   7. ENTROPY CODING AND HEADER.  The Annex K tables; restart_interval as in jpgpu_encode_params.  The header: SOI; APP0 "JFIF\0", version
 *     1.01, units 0, density 1 x 1, no thumbnail; DQT table 0 and DQT table 1, a segment each (one component: table 0 alone); SOF0, precision
 *     8, component identifiers 1, 2, 3, factors (H, V), (1, 1), (1, 1), tables 0, 1, 1; DHT DC0, AC0, DC1, AC1, a segment each (one
 *     component: the first two); DRI only with a restart interval, directly in front of SOS; SOS with selectors 0x00, 0x11, 0x11 and 00 3F 00.
 *   The blocks jpgpu_encoder_download_coefficients returns are the ones of steps 1 to 6, dummy blocks included.
 *   Refused, the encoder staying as it was: optimize_coding != 0 and luma factors other than the three shapes (JPGPU_ERR_ARGUMENT, for the
 * whole upload); jpgpu_encoder_upload_described and _upload_described_device (JPGPU_ERR_INVALID_OPERATION): a description is the
 * reference's encoder state.
 *   State of the encoder: every later jpgpu_encoder_upload / _upload_device reads it until it is set again; an upload keeps the arithmetic it
 * was planned with.  libjpeg's optimised tables and its progressive output are the coding policy's (4e).  Not covered: smoothing, other sampling
 * (4:4:0, 4:1:1), other segments (density, ICC, EXIF); the JpegEncoder mirror and the optimizer.
 * JPGPU_ERR_ARGUMENT for any other value of `policy` (a jpgpu_arithmetic_policy). */
int jpgpu_encoder_set_arithmetic_policy(jpgpu_encoder *e, int policy);
/* JPGPU_ARITHMETIC_LIBJPEG where image i of the last upload was planned with the integer transform, else JPGPU_ARITHMETIC_REFERENCE.  Valid
 * after an upload; JPGPU_ERR_ARGUMENT for a NULL argument or an index out of range. */
int jpgpu_encoder_image_arithmetic(const jpgpu_encoder *e, int i, int *arithmetic);
/* ---- (4e) Coding: libjpeg's optimal Huffman tables and its progressive mode (an extension beyond the reference; what Pillow's
 * Image.save(..., optimize=True) and Image.save(..., progressive=True) write).  Under JPGPU_ARITHMETIC_LIBJPEG only; steps 1 to 6 of (4d) and
 * the blocks jpgpu_encoder_download_coefficients returns are the same under all three codings.
 *   JPGPU_CODING_STANDARD, the default: every stream is what it was.
 *   JPGPU_CODING_OPTIMIZED: sequential SOF0 as in (4d) 7, with the DHT segments DC0, AC0 (, DC1, AC1) holding tables built from the image's
 * own symbols by the rule of jpgpu_libjpeg_optimal_table below.  restart_interval is honoured (the statistics see the same predictor resets).
 *   JPGPU_CODING_PROGRESSIVE: SOF2 with the scan script of jpeg_simple_progression.  The header is (4d)'s up to the frame header, SOF2 in
 * place of SOF0, nothing behind it.  Then per scan: one DHT segment per table the scan built, SOS, the scan's data; EOI.
 *     Three components, ten scans (component identifiers 1 = Y, 2 = Cb, 3 = Cr; Ss-Se, Ah, Al):
 *       1. DC of 1, 2, 3, Al = 1 (selectors 0x00, 0x10, 0x10; DHT DC0 and DC1 in front)      2. 1: 1-5, Al = 2       3. 3: 1-63, Al = 1
 *       4. 2: 1-63, Al = 1      5. 1: 6-63, Al = 2      6. 1: 1-63, Ah = 2, Al = 1      7. DC of 1, 2, 3, Ah = 1, Al = 0 (selectors 0, no DHT)
 *       8. 3: 1-63, Ah = 1, Al = 0      9. 2: 1-63, Ah = 1, Al = 0      10. 1: 1-63, Ah = 1, Al = 0
 *     One component, six scans: DC Al = 1; 1-5 Al = 2; 6-63 Al = 2; 1-63 Ah = 2 Al = 1; DC Ah = 1; 1-63 Ah = 1 Al = 0.
 *     Luma codes with table 0, chroma with table 1 (an AC scan: selector 0x00 / 0x01); every scan's tables are built from that scan alone.
 *     BLOCK ORDER.  A DC scan of three components is interleaved: MCU order, dummy blocks included.  An AC scan (and every scan of one
 *     component) visits the REAL blocks of its component, ceil(w_c / 8) x ceil(h_c / 8) in raster order.
 *     DC first: v = coef[0] >> Al (arithmetic), the difference to the component's previous v coded as in a sequential scan.  DC refinement:
 *     the bit (coef[0] >> Al) & 1 per block, no table.
 *     AC first, k over the band, t = |coef[k]| >> Al: t == 0: r++.  Else: flush the EOB run; ZRL (0xF0) while r > 15; symbol (r << 4) + nbits(t)
 *     and nbits bits (t, or ~t for a negative coefficient); r = 0.  At the block's end r > 0: EOBRUN++, flushed when it reaches 0x7FFF.
 *     AC refinement, abs[k] = |coef[k]| >> Al, EOB = the last k with abs == 1, r = BR = 0.  abs == 0: r++.  Else: while r > 15 && k <= EOB: flush,
 *     ZRL, r -= 16, the block's BR buffered bits, BR = 0.  abs > 1: buffer the bit abs & 1, BR++.  abs == 1: flush, symbol (r << 4) + 1, the sign
 *     bit (0: negative), the BR buffered bits, BR = r = 0.  At the block's end r > 0 || BR > 0: EOBRUN++, BE += BR, flushed when EOBRUN == 0x7FFF
 *     or BE > 937.
 *     A flush writes symbol n << 4 with n = floor(log2(EOBRUN)), the low n bits of EOBRUN, then the BE bits buffered by the run's blocks; the
 *     scan's end flushes.  Every scan ends padded with one-bits to a byte; FF is stuffed with 00.  The statistics take the same road.
 *     Files are those of progressive=True with or without optimize=True.
 *   Stages (jpgpu_encoder_stage_ms keeps five entries).  OPTIMIZED: the statistics kernel counts as stage E1, as under optimize_coding.
 * PROGRESSIVE: E1 as ever; ms[1] (E2) = block classification, run resolution and the statistics of all scans of all images (one copy to the
 * host and one table build per batch follow, not timed); ms[2] (E3) = bit counts, offsets and emission; ms[3] (E4) = byte stuffing per scan
 * and the assembly of header | (DHT, SOS, data) per scan | EOI in device memory (jpgpu_encoder_output_device works as ever).
 *   Output reservation: a scan's raw bit count is known exactly from its statistics before anything is written (sum of count x code length
 * plus the counted extra bits).  A scan's part of the file is at most its DHT and SOS segments + 2 x ceil(bits / 8) bytes (every byte
 * stuffed); the file is at most the frame header + the sum of these over its scans + 2 (EOI), and that is what is reserved for it, plus 64
 * bytes of slack, rounded up to 256 so that every file starts aligned.
 *   Refused at the upload with JPGPU_ERR_ARGUMENT, the encoder staying usable: a coding other than JPGPU_CODING_STANDARD while the arithmetic
 * policy is JPGPU_ARITHMETIC_REFERENCE (the reference's encoder has neither; its optimize_coding stays what it is), and JPGPU_CODING_PROGRESSIVE
 * with restart_interval != 0.  optimize_coding != 0 under JPGPU_ARITHMETIC_LIBJPEG and the described uploads keep the refusals of (4d).
 *   State of the encoder like the arithmetic policy: later uploads read it until it is set again, an upload keeps what it was planned with.
 *   Out of scope: progressive with restart intervals, custom scan scripts, the JpegEncoder mirror and described uploads, JPGPU_ARITHMETIC_REFERENCE,
 * the optimizer.
 * JPGPU_ERR_ARGUMENT for any other value of `policy`. */
typedef enum jpgpu_coding_policy {
    JPGPU_CODING_STANDARD = 0,   /* the Annex K tables, sequential */
    JPGPU_CODING_OPTIMIZED = 1,  /* sequential, tables built from the image by libjpeg's rule */
    JPGPU_CODING_PROGRESSIVE = 2 /* SOF2, jpeg_simple_progression, a table built per scan */
} jpgpu_coding_policy;
int jpgpu_encoder_set_coding_policy(jpgpu_encoder *e, int policy);
/* The jpgpu_coding_policy image i of the last upload was planned with.  JPGPU_ERR_ARGUMENT for a NULL argument or an index out of range. */
int jpgpu_encoder_image_coding(const jpgpu_encoder *e, int i, int *coding);
/* Host only, no context, no device: libjpeg's jpeg_gen_optimal_table.  freq[256] are a table's symbol counts.  A pseudo-symbol 256 of count 1
 * joins them, so that no code is all ones.  Repeat: c1 = the symbol of the least non-zero count, among equals the LARGEST index; c2 the next
 * least by the same rule; freq[c1] += freq[c2], freq[c2] = 0, one bit more for every symbol on both chains, the chains linked.  Count the code
 * sizes (up to 32), then limit them to 16: for i = 32 .. 17, while bits[i] > 0: j = i - 2 stepping down to the first bits[j] != 0; bits[i] -= 2,
 * bits[i - 1]++, bits[j + 1] += 2, bits[j]--.  The pseudo-symbol leaves the longest non-empty length.  bits16[l - 1] = codes of length l;
 * values[0 .. *n_values) = the symbols by code size, then by value (a histogram of one symbol gives it a 1-bit code).  A histogram of
 * nothing but zeros gives the empty table: JPGPU_OK, sixteen zero counts, *n_values = 0, values untouched.
 * JPGPU_ERR_ARGUMENT for a NULL argument. */
int jpgpu_libjpeg_optimal_table(const uint32_t freq[256], uint8_t bits16[16], uint8_t values[256], int *n_values);
/* status of image i as known so far (after the upload: JPGPU_OK or the refusal; after the encode also "No symbol is recorded.") */
int jpgpu_encoder_image_status(const jpgpu_encoder *e, int i);
/* Host only, no context, no device: the status an encode of `desc` would report, with its message in message[message_cap]
 * (may be NULL), and -- for a description without tables to be built -- the SOI, DQT, (DRI,) SOF0, DHT, SOS bytes Encode()
 * writes in front of the scan (*len; JPGPU_ERR_ARGUMENT when cap is too small, *len still set).  With tables to be built the
 * DHT depends on the image: *len = 0.  JPGPU_ERR_INVALID_OPERATION: a table to be built that no component feeds. */
int jpgpu_encode_description_header(const jpgpu_encode_description *desc, uint8_t *dst, size_t cap, size_t *len, char *message,
                                    size_t message_cap);

/* ------------------------------------------------------------------------------------------------
 * (5) Optimizer -- replaces JpegOptimizer (ref: JpegOptimizer.cs) for single-scan baseline files:
 *     SetInput (:57-63) + Scan() (:66-153) + SetOutput (:523-526) + Optimize(strip) (:540-648).  The marker walks run on
 *     the host, the two symbol passes (ProcessScanBaseline :360-463, CopyScanBaseline :719-829) on the device, the new
 *     Huffman tables are JpegHuffmanEncodingTableBuilder.Build(false) (JpegHuffmanEncodingTableBuilder.cs:68-175).
 *     Not supported (JPGPU_ERR_NOT_SUPPORTED): more than one scan, progressive frames.
 * ---------------------------------------------------------------------------------------------- */
typedef struct jpgpu_optimizer jpgpu_optimizer;
int jpgpu_optimizer_create(jpgpu_ctx *ctx, jpgpu_optimizer **out);
void jpgpu_optimizer_destroy(jpgpu_optimizer *o);
/* SetInput for n files (host marker walks + H2D); strip = Optimize(strip)'s argument */
int jpgpu_optimizer_upload(jpgpu_optimizer *o, const uint8_t *const *jpeg, const size_t *len, int n, int strip);
/* JpegOptimizer.MostOptimalCoding (:38): Build(optimal = true), the package-merge builder */
int jpgpu_optimizer_set_most_optimal_coding(jpgpu_optimizer *o, int on);
/* Scan() + Optimize(strip) for every file */
int jpgpu_optimizer_run(jpgpu_optimizer *o);
/* status of file i with the reference's exception classes; out_len = bytes Optimize() wrote */
int jpgpu_optimizer_result(jpgpu_optimizer *o, int i, jpgpu_image_result *res, size_t *out_len);
int jpgpu_optimizer_download(jpgpu_optimizer *o, int i, void *dst, size_t cap);  /* the IBufferWriter's content */
/* what Scan() counted for table `table` of file i, in the order the reference creates its table builders (:381-413) */
int jpgpu_optimizer_statistics(const jpgpu_optimizer *o, int i, int table, uint8_t *table_class, uint8_t *identifier, uint32_t *counts);
int jpgpu_optimizer_last_ms(const jpgpu_optimizer *o, float *ms);  /* device time of the last run (HIP events) */

/* ---- Lossless transform: an image is turned or flipped in the coefficient domain on its way through the optimizer (an extension beyond the
 * reference; what jpegtran -rotate / -flip / -transpose -optimize -copy none and exiftran -a do).  No coefficient is requantised.
 *   Inputs.  The files the optimizer accepts: one sequential Huffman scan.  Progressive and multi-scan files stay JPGPU_ERR_NOT_SUPPORTED; the
 * fences of DESIGN.md 5 apply as they are.  Refused per image with JPGPU_ERR_NOT_SUPPORTED when it is to be turned: a scan that does not hold
 * every component of the frame once, in frame order; more than four components; factors outside 1..4; a one-component frame whose factors are
 * not 1 x 1; a scan component without a Huffman table.
 *   Orientation of an image: the decoder's vocabulary ("Orientation" above), unchanged.  jpgpu_optimizer_set_orientation_policy is state of
 * the optimizer (JPGPU_ORIENT_STORED, the default, or JPGPU_ORIENT_FILE with the Exif rule of jpgpu_identify_orientation);
 * jpgpu_optimizer_set_orientations gives the NEXT upload one value per file and is consumed by it: 1..8 is used as given, 0 leaves the image
 * to the policy, n == 0 withdraws a pending list.  JPGPU_ERR_ARGUMENT for a value above 8 or an unknown policy; an upload whose n differs from
 * the list's is refused with JPGPU_ERR_ARGUMENT and leaves the optimizer empty.
 *   Orientation 1: the image takes the transcode path above; its bytes and its status are what the optimizer gives without any of this.  With
 * no list pending under JPGPU_ORIENT_STORED, or with a 1 in the list, the file is not looked at for the transform at all.  Otherwise its
 * headers up to the first SOS are read by Identify()'s marker loop -- the one jpgpu_identify_orientation runs: markers are looked for, not
 * expected, lengths follow the reference's rule --, and a file that loop cannot walk is not turned: it keeps what the optimizer makes of it.
 *   Orientations 2..8.  With F the source file, whose MCU is 8 Hmax x 8 Vmax pixels, the output is Optimize(strip) of a file F' that differs
 * from F in four things.
 *   1. Blocks.  The decoded picture of F' is the picture of F under the source-pixel table of "Orientation", (Y, X) <- (y, x).  Per block, with
 *     c[v][u] the de-zig-zagged coefficients and v the vertical frequency: a mirror in x negates every odd u, a mirror in y every odd v, and a
 *     transposing orientation (5..8) swaps u and v.  Source x is mirrored for 2, 3, 7, 8, source y for 3, 4, 6, 7.  Blocks move inside each
 *     component's full MCU-padded grid: output block (bx', by') of a component is source block (bx, by) under the same table in units of
 *     blocks, so padding blocks of the source land on padding positions of the output with whatever they hold (no dummy-block rule of libjpeg's
 *     is adopted).  Values are never clamped or requantised; -(-32768) stays -32768.
 *   2. SOF.  For 5..8 width and height are swapped and every component's H and V nibbles are swapped (4:2:2 becomes 4:4:0, 4:1:1 becomes
 *     1 x 4).  Component ids and table selectors are unchanged.
 *   3. DQT.  For 5..8 every table is transposed in place in its segment: entry zz(v, u) takes the value of entry zz(u, v), 8- and 16-bit
 *     entries alike.  Segment order and lengths are unchanged.
 *   4. DRI.  The value is kept: restart markers follow every DRI MCUs of the NEW MCU order, and DC prediction restarts there.
 *   Huffman tables.  Optimize(strip) depends only on the segments and the symbol sequence, so the Huffman coding of F' does not matter: the
 * output's tables are JpegHuffmanEncodingTableBuilder.Build over the statistics of the TURNED blocks, per (class, identifier) in the order the
 * source declares them; jpgpu_optimizer_set_most_optimal_coding is honoured.  (The marker search of Optimize() runs through the DHT payloads:
 * the source's are assumed to hold no FF byte, as those of every valid table.)
 *   Edges.  A mirrored source axis must be a whole number of source MCUs.  Otherwise, under JPGPU_EDGE_REFUSE (the default; jpegtran -perfect)
 * that image alone reports JPGPU_ERR_NOT_SUPPORTED with a message naming the axis, and its output length is 0; under JPGPU_EDGE_TRIM (jpegtran
 * -trim) the partial last MCU column or row of the mirrored axis is dropped before the transform -- the width or height becomes the largest
 * multiple of the MCU size --, and an axis shorter than one MCU is refused as above.  Non-mirrored axes are never trimmed; 5 needs nothing.
 *   Exif.  Without `strip`, when the applied orientation came from the file under the policy (not from the list) and is not 1, the two bytes of
 * the tag the identify rule found are rewritten to 1 in the file's byte order.  Nothing else in any APPn changes: thumbnails and the
 * pixel-dimension tags inside Exif are out of scope and keep what the source says.
 *   Failing scans.  An image whose scan the optimizer would fail keeps that status; its output is empty and its neighbours are untouched.
 * The reference's restart rule holds for F' as for any file: where the MCU count of F' is a multiple of DRI, Scan() returns before it builds
 * its tables and the image reports JPGPU_ERR_INVALID_OPERATION (a trimmed image has fewer MCUs than its source).
 *   jpgpu_optimizer_image_transform reports, after an upload, what image i was planned with: applied orientation, output size, whether it was
 * trimmed, the per-component factors of the output.  jpgpu_transform_plan gives the same facts and the refusal from a file alone -- host
 * only, no context, no device -- as jpgpu_encode_description_header does for the encoder: `orientation` 0 = by `policy`, 1..8 as given; the
 * return value is JPGPU_OK, the refusal (its text in message[message_cap], may be NULL), or the library's header error.  It reads the headers
 * up to the first SOS as described under "Orientation 1": a second scan is the upload's to refuse.
 *   Window (what jpegtran -crop does).  jpgpu_optimizer_set_windows gives the NEXT upload one jpgpu_rect per file and is consumed by it, as
 * the orientations are: n == 0 withdraws a pending list, an upload whose n differs is refused with JPGPU_ERR_ARGUMENT and leaves the optimizer
 * empty.  {0, 0, 0, 0} means no window: with orientation 1 the file is then not looked at and keeps the transcode path, its bytes and its
 * status.  Any other window -- the whole frame written out included -- takes the coefficient road, turned or not.
 *     What the output is.  With F' the turned file as defined above (F itself where the applied orientation is 1), the output is
 *   Optimize(strip) of a file F'' that differs from F' in two things.  Blocks: with (mw, mh) the MCU size of F' in pixels and the window
 *   (x, y, w, h) in pixels of the frame of F' -- the turned frame, behind a trim, exactly as the decoder's windows are in pixels of the oriented
 *   frame --, F'' holds the MCUs of F' from MCU column x / mw and MCU row y / mh on, ceil(w / mw) columns and ceil(h / mh) rows of them; every
 *   block holds what it held in F', and where the window reaches the edge of F' its padding blocks come along as they are.  SOF: the size
 *   becomes w x h.  Everything else is that of F': factors and DQT (transposed for 5..8), DRI (kept), the Exif rewrite, the Huffman rule,
 *   everything behind the scan.  Statistics are taken from the blocks of F'' only.  Decoding F'' gives, sample for sample, the slice
 *   [y, y + h) x [x, x + w) of the decode of F'.
 *     Order.  The orientation and the edge policy are resolved on the whole frame first, exactly as without a window: a mirrored axis that is
 *   no whole number of MCUs still refuses or trims the image, even if the window would leave that edge out.  Then the window is applied.
 *     Origin.  x must be a multiple of mw and y a multiple of mh.  Under JPGPU_ORIGIN_REFUSE (the default; jpegtran -perfect) a window that
 *   breaks this refuses that image alone with JPGPU_ERR_NOT_SUPPORTED and a message naming the coordinate and the MCU size; under
 *   JPGPU_ORIGIN_EXPAND (jpegtran's default) x drops to the multiple below and w grows by the difference, y and h likewise.  w and h are free.
 *   jpgpu_optimizer_set_origin_policy is state of the optimizer; JPGPU_ERR_ARGUMENT for another value.
 *     Refusals.  A window that does not lie inside the frame of F', or with exactly one of w, h zero, fails that image alone with
 *   JPGPU_ERR_ARGUMENT (the decoder's rule and status): its output length is 0 and its neighbours are untouched.  An image with a window is
 *   refused for the reasons a turned one is (progressive, several scans, more than ten blocks per MCU, ...).  Where the headers cannot be
 *   walked at all and the file has a window, the image FAILS with the plan's header error -- unlike the turn's rule ("is not turned"): a
 *   caller who asked for a region never gets the whole picture back silently.
 *     Restart rule.  It is that of F'': where ITS MCU count is a multiple of DRI the image reports JPGPU_ERR_INVALID_OPERATION, and the MCU
 *   count of the source does not decide it.
 *     One decode per source.  Entries of one upload that are the same file (the same pointer and length) are entropy-decoded once for the
 *   coefficient road; jpgpu_optimizer_turn_sources reports how many files the last upload decoded for it.  Outputs do not depend on it.
 *     jpgpu_optimizer_image_window reports the window image i was planned with, behind JPGPU_ORIGIN_EXPAND ({0, 0, W', H'} for an image
 *   without one), and jpgpu_optimizer_image_transform then reports the OUTPUT size w x h.  jpgpu_transform_plan_window is
 *   jpgpu_transform_plan with the window (`applied` may be NULL); a NULL or all-zero window gives exactly what jpgpu_transform_plan gives.
 *   Not covered: several windows into one output, jpegtran's rule that a window may rescue a partial mirrored edge (the edge policy is resolved
 * on the whole frame), jpegtran's default of leaving an unmirrored strip at the edge, grey-scale conversion, Exif pixel-dimension tags and
 * thumbnails, the JpegOptimizer mirror. */
typedef enum jpgpu_edge_policy {
    JPGPU_EDGE_REFUSE = 0, /* a mirrored axis that is no whole number of MCUs refuses the image */
    JPGPU_EDGE_TRIM = 1    /* ... drops its partial last MCU column or row */
} jpgpu_edge_policy;
typedef struct jpgpu_transform_info {
    int32_t orientation;    /* applied: 1..8 */
    int32_t trimmed;        /* 1: an edge was dropped */
    uint32_t width, height; /* of the output */
    uint32_t num_components;
    uint8_t h[4], v[4];     /* of the output, frame order */
    uint32_t reserved;
} jpgpu_transform_info;
size_t jpgpu_sizeof_transform_info(void);
int jpgpu_optimizer_set_orientation_policy(jpgpu_optimizer *o, int policy);
int jpgpu_optimizer_set_orientations(jpgpu_optimizer *o, const uint8_t *orientations, int n);
int jpgpu_optimizer_set_edge_policy(jpgpu_optimizer *o, int edge);
int jpgpu_optimizer_image_transform(const jpgpu_optimizer *o, int i, jpgpu_transform_info *info);
/* the turned images' road in the last run (zeros: nothing was turned), HIP events on the context's stream: ms[0] KX alone, ms[1] the entropy
 * decode in front of it, ms[2] the dense copy of the scans K2 handed over as half-line planes (tools/bench_transform.py reads them) */
int jpgpu_optimizer_turn_ms(const jpgpu_optimizer *o, float ms[3]);
int jpgpu_transform_plan(const uint8_t *file, size_t len, int orientation, int policy, int edge, jpgpu_transform_info *info, char *message,
                         size_t message_cap);
/* ... and the window ("Window" above) */
typedef enum jpgpu_origin_policy {
    JPGPU_ORIGIN_REFUSE = 0, /* a window whose x or y is no multiple of the MCU size refuses the image */
    JPGPU_ORIGIN_EXPAND = 1  /* ... is moved up and left to the MCU boundary, and grows by as much */
} jpgpu_origin_policy;
int jpgpu_optimizer_set_origin_policy(jpgpu_optimizer *o, int origin);
int jpgpu_optimizer_set_windows(jpgpu_optimizer *o, const jpgpu_rect *windows, int n);
int jpgpu_optimizer_image_window(const jpgpu_optimizer *o, int i, jpgpu_rect *applied);
int jpgpu_optimizer_turn_sources(const jpgpu_optimizer *o, int *files);
int jpgpu_transform_plan_window(const uint8_t *file, size_t len, int orientation, int policy, int edge, const jpgpu_rect *window, int origin,
                                jpgpu_transform_info *info, jpgpu_rect *applied, char *message, size_t message_cap);

/* JpegHuffmanEncodingTableBuilder.Build(false) for one table: DHT counts and values, and GetCode() for all 256 symbols */
/* The order .NET's Array.Sort(T[], Comparison<T>) / List<T>.Sort(Comparison<T>) leaves n elements in when the comparison looks at
 * an int32 key alone (ascending): perm[i] = original index of the element that ends up at position i.  That sort is not stable,
 * and the reference orders equal-length symbols (JpegHuffmanEncodingTableBuilder.cs:171) and its package-merge nodes (:352,
 * :374, :395) with it, so the DHT bytes the optimizer and the encoder write depend on the runtime's algorithm (restated from
 * ArraySortHelper<T>.IntrospectiveSort).  Exposed so that the restatement can be held against independent ones. */
int jpgpu_net_sort_permutation(const int32_t *keys, int n, int32_t *perm);
int jpgpu_build_optimal_huffman_table(const uint32_t *counts, int most_optimal, uint8_t *bits, uint8_t *values, int *num_values,
                                      uint16_t *code, uint8_t *length);

#ifdef __cplusplus
}
#endif
#endif /* JPGPU_H */
