/* zoe_sw.h — C ABI of the MI355X (gfx950) implementation of Zoe's striped Smith-Waterman hot path.
 *
 * CDCgov/zoe is a pure-Rust crate with no FFI of its own; the boundary this header replaces is the
 * set of generic Rust functions below (file:line in the reference checkout).  Each entry point is the
 * *batched* form of one of them: "for every read i: build the profile from read i, run the function
 * against the context's reference".  Role convention (src/alignment/sw/mod.rs:119-120): the read is
 * the profile sequence ("query"), the context's sequence is `reference`.
 *
 *   StripedProfile::<T,N,S>::new(seq,&matrix,go,ge)          src/alignment/profile.rs:239-247
 *   sw_simd_score::<T,N,S>(reference,&profile)               src/alignment/sw/striped.rs:65-142
 *   sw_simd_score_ends::<T,N,S>(reference,&profile)          src/alignment/sw/striped.rs:153-162
 *   sw_simd_align::<T,N,S>(reference,&profile)               src/alignment/sw/striped.rs:449-598
 *   ProfileSets::sw_score_from_{i8,i16,i32}                  src/alignment/profile_set.rs:71-107
 *   ProfileSets::sw_align_from_{i8,i16,i32}                  src/alignment/profile_set.rs:124-179
 *   LocalProfiles::new_with_w{128,256,512}                   src/alignment/profile_set.rs:434-483
 *   Nucleotides::into_local_profile (w256)                   src/data/types/nucleotides/mod.rs:262-266
 *   SeqSrc::make_alignment / Alignment::invert               src/alignment/mod.rs:176-190, types/output.rs:396-425
 *
 * Plain pointers and sizes only; no hidden global state; one context per GPU (zsw_group for several); a context may
 * be used from one host thread at a time, and from one stream at a time: consecutive asynchronous calls on the same stream are
 * ordered, calls on two streams must not overlap on one context.  Every function returns a zsw_error and never aborts.  A call leaves the
 * calling thread's current HIP device as it found it.  At most 2^31-1 reads per call.
 * Results are bit-identical to the reference's CPU path: score and status for every read; for the
 * alignment calls also ranges and CIGAR of the stated <T,N> instantiation.
 */
#ifndef ZOE_SW_H
#define ZOE_SW_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Codes 1..4 are ProfileError (src/alignment/errors.rs:6-15) as raised by validate_profile_args
 * (src/alignment/profile.rs:32-44). */
typedef enum zsw_error {
    ZSW_OK = 0,
    ZSW_ERR_EMPTY_SEQUENCE = 1,
    ZSW_ERR_GAP_OPEN_OUT_OF_RANGE = 2,
    ZSW_ERR_GAP_EXTEND_OUT_OF_RANGE = 3,
    ZSW_ERR_BAD_GAP_WEIGHTS = 4,
    ZSW_ERR_INVALID_ARGUMENT = -1,
    ZSW_ERR_HIP = -2,          /* a HIP runtime call failed; see zsw_last_error_string */
    ZSW_ERR_NO_DEVICE = -3,    /* no gfx950 device / HIP runtime unusable: the product path fails loudly */
    ZSW_ERR_UNSUPPORTED = -4,  /* valid in the reference but outside what the kernels cover (documented) */
    ZSW_ERR_NOT_CONFIGURED = -5
} zsw_error;

/* MaybeAligned<T> (src/alignment/types/output.rs:18-25), per read. ZSW_STATUS_EMPTY marks a read of
 * length 0, for which StripedProfile::new returns Err(ProfileError::EmptySequence). ZSW_STATUS_BELOW_MIN_SCORE is reported
 * only while ZSW_OPTION_MIN_SCORE is set (below): the read scores less than the caller's minimum; every other field of it is 0. */
typedef enum zsw_status {
    ZSW_STATUS_SOME = 0,
    ZSW_STATUS_OVERFLOWED = 1,
    ZSW_STATUS_UNMAPPED = 2,
    ZSW_STATUS_EMPTY = 3,
    ZSW_STATUS_BELOW_MIN_SCORE = 4
} zsw_status;

/* The most members a reference panel holds (zsw_set_panel, below) */
#define ZSW_PANEL_MAX_REFS 64

/* T of StripedProfile<T,N,S> (AlignableIntWidth, src/math/integer.rs:231-238). Unsigned types run
 * the biased algorithm on matrix.to_biased_matrix() (src/data/matrices/mod.rs:471-491). */
typedef enum zsw_int_type { ZSW_I8 = 0, ZSW_I16 = 1, ZSW_I32 = 2, ZSW_U8 = 3, ZSW_U16 = 4, ZSW_U32 = 5 } zsw_int_type;

typedef enum zsw_mem { ZSW_MEM_HOST = 0, ZSW_MEM_DEVICE = 1 } zsw_mem;

typedef struct zsw_context zsw_context;

/* A batch of profile sequences (reads). Either fixed-length (offsets == NULL, read i occupies
 * bases[i*fixed_len, (i+1)*fixed_len)) or ragged (offsets[n_reads+1], read i = bases[offsets[i], offsets[i+1])).
 * `mem` says where bases/offsets AND the output arrays of the call live. */
/* How `bases` spells the reads. ZSW_ENCODING_BYTES (0, the default): one byte per base, as in a Nucleotides buffer.
 * ZSW_ENCODING_PACKED4: two bases per byte as residue indices of the context's ByteIndexMap (index_map[byte], < 16), the first
 * base of a pair in the low nibble; read i occupies bases[i * ((fixed_len + 1) / 2) ...]. Fixed-length host batches only: a shard
 * that crosses PCIe at half the bytes (zsw_pack4_host packs a byte batch; the library unpacks on the device). */
typedef enum zsw_encoding { ZSW_ENCODING_BYTES = 0, ZSW_ENCODING_PACKED4 = 1 } zsw_encoding;

typedef struct zsw_batch {
    const uint8_t* bases;
    const uint64_t* offsets;
    uint32_t fixed_len;
    uint64_t n_reads;
    zsw_mem mem;
    zsw_encoding encoding;
} zsw_batch;

/* Per-read alignment record: Alignment<u32> (src/alignment/types/output.rs:264-279) with
 * AlignmentStates (src/alignment/types/state.rs:53) flattened into a ciglet array. */
typedef struct zsw_alignment {
    uint32_t score;
    uint32_t ref_start, ref_end;     /* ref_range   (0-based, end-exclusive) */
    uint32_t query_start, query_end; /* query_range (excludes clipped bases) */
    uint32_t ref_len, query_len;
    uint32_t n_ciglets;              /* number of (inc, op) pairs of this read */
    uint64_t ciglet_offset;          /* index of its first pair in the ciglet arrays */
} zsw_alignment;

/* ---- context ------------------------------------------------------------------------------- */
/* Host utility: packs n_reads reads of `len` bytes each (contiguous) into ZSW_ENCODING_PACKED4 with the context's ByteIndexMap
 * (zsw_set_scoring first; alphabets of up to 16 letters); out_packed: n_reads * ((len + 1) / 2) bytes. No GPU work. */
zsw_error zsw_pack4_host(zsw_context* ctx, const uint8_t* bases, uint64_t n_reads, uint32_t len, uint8_t* out_packed);

zsw_error zsw_create(int device_id, zsw_context** out);
void zsw_destroy(zsw_context* ctx);
/* The message of the context's last failing call. ctx == NULL: why the last zsw_create of the CALLING THREAD failed
 * (thread-local; no state is shared between threads). */
const char* zsw_last_error_string(const zsw_context* ctx);
int zsw_device_count(void);

/* WeightMatrix<i8,S> + ByteIndexMap<S> + gap penalties, validated exactly like validate_profile_args
 * (codes 2..4). weights[r*S + q]: row = reference residue, column = query residue
 * (src/data/matrices/mod.rs:242-244); index_map[256] = ByteIndexMap::to_index
 * (src/data/constants/mappings/byte_index.rs:331-333); 1 <= S <= 32. */
zsw_error zsw_set_scoring(zsw_context* ctx, const int8_t* weights, int S, const uint8_t* index_map, int gap_open,
                          int gap_extend);

/* The `reference: &[u8]` argument of sw_simd_*; copied into the context (replicated per GPU).
 * zsw_set_reference and zsw_set_scoring wait for the device to finish the work already queued (asynchronous score calls on
 * any stream may still be reading the previous tables) before they overwrite them; they are configuration calls, not
 * per-batch calls. */
zsw_error zsw_set_reference(zsw_context* ctx, const uint8_t* reference, size_t len, zsw_mem mem);

/* ---- score-only ---------------------------------------------------------------------------- */
/* out_score[i], out_status[i] = StripedProfile::<int_type, lanes, S>::new(read_i).sw_score(reference).
 * `lanes` must be a power of two in 2..64 (it does not change a score; it is checked and kept for
 * signature parity). `stream` is a hipStream_t (NULL = default stream); the call is asynchronous
 * when batch.mem == ZSW_MEM_DEVICE. */
zsw_error zsw_score_batch(zsw_context* ctx, const zsw_batch* reads, zsw_int_type int_type, int lanes,
                          uint32_t* out_score, uint8_t* out_status, void* stream);

/* LocalProfiles::new_with_w{preset_bits}(read_i).sw_score_from_i{from_width}(reference):
 * from_width in {8,16,32}, preset_bits in {128,256,512}. out_tier (optional) = width that answered. */
zsw_error zsw_score_batch_from(zsw_context* ctx, const zsw_batch* reads, int from_width, int preset_bits,
                               uint32_t* out_score, uint8_t* out_status, uint8_t* out_tier, void* stream);

/* ---- score + ends -------------------------------------------------------------------------- */
/* sw_simd_score_ends: 0-based exclusive ends; first row holding the maximum, then first column. */
zsw_error zsw_score_ends_batch(zsw_context* ctx, const zsw_batch* reads, zsw_int_type int_type, int lanes,
                               uint32_t* out_score, uint32_t* out_ref_end, uint32_t* out_query_end,
                               uint8_t* out_status, void* stream);

/* sw_simd_score_ranges (src/alignment/sw/striped.rs:355-388): the truncated two-pass form — forward score+ends, then
 * sw_simd_score_ends_reverse on reference[..ref_end] with the profile of reverse(read[..query_end]). Ranges are
 * 0-based half-open. */
zsw_error zsw_score_ranges_batch(zsw_context* ctx, const zsw_batch* reads, zsw_int_type int_type, int lanes,
                                 uint32_t* out_score, uint32_t* out_ref_start, uint32_t* out_ref_end,
                                 uint32_t* out_query_start, uint32_t* out_query_end, uint8_t* out_status, void* stream);

/* ProfileSets::sw_score_ranges_from_i{8,16,32} (src/alignment/profile_set.rs:313-362): the cascade over the tiers of the
 * w{preset_bits} preset; out_tier (optional) = width that answered. */
zsw_error zsw_score_ranges_batch_from(zsw_context* ctx, const zsw_batch* reads, int from_width, int preset_bits,
                                      uint32_t* out_score, uint32_t* out_ref_start, uint32_t* out_ref_end,
                                      uint32_t* out_query_start, uint32_t* out_query_end, uint8_t* out_status, uint8_t* out_tier,
                                      void* stream);

/* ---- full alignment ------------------------------------------------------------------------ */
/* out_aln[i] / out_status[i] = StripedProfile::<int_type,lanes,S>::new(read_i).sw_align(SeqSrc::Reference(reference))
 * (invert != 0: SeqSrc::Query(reference), i.e. the result passed through Alignment::invert).
 * Ciglets of all reads are packed into out_inc/out_op (capacity ciglet_cap pairs); *out_n_ciglets
 * receives the total. If the capacity is too small the call returns ZSW_ERR_INVALID_ARGUMENT and
 * *out_n_ciglets holds the required size. This call synchronises the stream. */
zsw_error zsw_align_batch(zsw_context* ctx, const zsw_batch* reads, zsw_int_type int_type, int lanes, int invert,
                          zsw_alignment* out_aln, uint8_t* out_status, uint32_t* out_inc, uint8_t* out_op,
                          uint64_t ciglet_cap, uint64_t* out_n_ciglets, void* stream);

/* LocalProfiles::new_with_w{preset_bits}(read_i).sw_align_from_i{from_width}(..): each read's CIGAR is
 * that of the first tier that does not overflow (each tier has its own lane count). */
zsw_error zsw_align_batch_from(zsw_context* ctx, const zsw_batch* reads, int from_width, int preset_bits, int invert,
                               zsw_alignment* out_aln, uint8_t* out_status, uint8_t* out_tier, uint32_t* out_inc,
                               uint8_t* out_op, uint64_t ciglet_cap, uint64_t* out_n_ciglets, void* stream);

/* ---- 3-pass alignment ---------------------------------------------------------------------- */
/* sw_align_3pass (src/alignment/sw/three_pass.rs:21-104; profile.rs:546-552): score ranges first, then the no-gaps shortcut,
 * a doubling banded alignment (sw/banded.rs:40-133) or the scalar alignment (sw/scalar.rs:173-271) inside the bounding box.
 * Same outputs as zsw_align_batch; like in the reference the CIGAR may differ from sw_simd_align's where several optimal
 * alignments exist (the score and validity do not). */
zsw_error zsw_align_3pass_batch(zsw_context* ctx, const zsw_batch* reads, zsw_int_type int_type, int lanes, int invert,
                                zsw_alignment* out_aln, uint8_t* out_status, uint32_t* out_inc, uint8_t* out_op,
                                uint64_t ciglet_cap, uint64_t* out_n_ciglets, void* stream);
/* ProfileSets::sw_align_from_i{8,16,32}_3pass (src/alignment/profile_set.rs:212-283) */
zsw_error zsw_align_3pass_batch_from(zsw_context* ctx, const zsw_batch* reads, int from_width, int preset_bits, int invert,
                                     zsw_alignment* out_aln, uint8_t* out_status, uint8_t* out_tier, uint32_t* out_inc,
                                     uint8_t* out_op, uint64_t ciglet_cap, uint64_t* out_n_ciglets, void* stream);

/* ---- reads from either strand -------------------------------------------------------------- */
/* Reads from a sequencer come from both strands; about half of them match the reference only as their reverse complement
 * (Nucleotides::to_reverse_complement, src/data/types/nucleotides/mod.rs; the "Reversibility" notes on Alignment,
 * src/alignment/types/output.rs:233-256). With rc(read) = the read reversed, every byte sent through the context's complement
 * table, and f one of the entry points above: F_i = f(read_i), R_i = f(rc(read_i)). The strand-aware result of read i is F_i
 * unless R_i ranks strictly higher — ZSW_STATUS_OVERFLOWED > ZSW_STATUS_SOME by score > ZSW_STATUS_UNMAPPED = ZSW_STATUS_EMPTY;
 * ties go to the forward strand. out_strand[i] = 0 (forward) or 1 (reverse); everything else of the result is bit for bit
 * what f returns for the chosen orientation, with coordinates in the sequence as aligned, i.e. in rc(read_i) for strand 1:
 * what a SAM record with flag 16 carries.
 * The library does not score both orientations of every read: k-mers of both orientations looked up in the
 * reference index bound what either orientation can score at all, the more promising one is scored first, and the other one
 * only if that bound does not already rank it below. Same results for every input; ZSW_OPTION_EXACT_PRUNING = 0, or a matrix or
 * reference the index cannot serve, scores every read on both strands.
 * Not covered: zsw_group_*, the direct (one <T, N>) calls, the ends and ranges calls, the shared-profile role — orient the reads
 * with zsw_orient_batch once the strands are known and use any entry point on the oriented batch. */

/* Optional. table[b] = the byte of the base complementary to byte b. NULL restores the default: the IUPAC nucleotide complement
 * (A<->T, C<->G, U->A, R<->Y, K<->M, B<->V, D<->H; S, W, N themselves), case preserved, every other byte mapped to itself. */
zsw_error zsw_set_complement(zsw_context* ctx, const uint8_t* table /* 256 entries */);

/* zsw_score_batch_from under the contract above; out_tier is optional, out_strand is not. Host and device batches, fixed and
 * ragged, ZSW_ENCODING_BYTES; ZSW_ENCODING_PACKED4 returns ZSW_ERR_UNSUPPORTED (a packed residue index has no complement byte).
 * The call synchronises the stream once, to read the number of reads that need their other strand scored (and, like every call,
 * once more for a ragged device batch, whose size comes back from the device). Device workspace: the oriented copy of the batch,
 * a second batch of the reads scored on both strands, 8 bytes per read — for a host batch also the staged batch itself, three
 * times its bytes in all; kept by the context until zsw_destroy or zsw_set_option(ZSW_OPTION_EXACT_PRUNING, 0).
 * A host batch crosses PCIe whole, in one copy, before the first kernel: the chunked copies that zsw_score_batch_from overlaps with
 * its kernels for large fixed-length host batches are not used here (not measured; keep large batches on the device). */
zsw_error zsw_score_strands_batch_from(zsw_context* ctx, const zsw_batch* reads, int from_width, int preset_bits,
                                       uint32_t* out_score, uint8_t* out_status, uint8_t* out_tier, uint8_t* out_strand, void* stream);

/* out_bases = the batch with every read i of strand[i] != 0 replaced by rc(read_i), the others copied: the same layout and the same
 * offsets as the input, in host or device memory as the input (strand and out_bases live where reads->mem says; out_bases must
 * not overlap reads->bases). Needs neither scoring nor reference. ZSW_ENCODING_PACKED4 returns ZSW_ERR_UNSUPPORTED. Applying it
 * twice with the same strands restores the input if the complement table is an involution (the default is, but for U). */
zsw_error zsw_orient_batch(zsw_context* ctx, const zsw_batch* reads, const uint8_t* strand, uint8_t* out_bases, void* stream);

/* zsw_align_3pass_batch_from under the contract above: the strand decision of zsw_score_strands_batch_from, then ONE alignment run
 * on the oriented batch. Arguments as zsw_align_3pass_batch_from, plus out_strand. */
zsw_error zsw_align_3pass_strands_batch_from(zsw_context* ctx, const zsw_batch* reads, int from_width, int preset_bits, int invert,
                                             zsw_alignment* out_aln, uint8_t* out_status, uint8_t* out_tier, uint8_t* out_strand,
                                             uint32_t* out_inc, uint8_t* out_op, uint64_t ciglet_cap, uint64_t* out_n_ciglets, void* stream);

/* Counters of the context's last strand-aware call: out[0] reads settled on the forward strand by proof (the reverse strand was
 * never scored), out[1] settled on the reverse strand by proof, out[2] scored on both strands, out[3] answered as reverse.
 * out[0] + out[1] + out[2] = the reads of the call. Synchronises the device. */
zsw_error zsw_strand_counts(zsw_context* ctx, uint64_t* out /* 4 entries */);

/* ---- reference panels: the best of several references -------------------------------------- */
/* A panel is n_refs sequences r_0 .. r_{n_refs-1}, 1 <= n_refs <= ZSW_PANEL_MAX_REFS — the segments and subtypes of a virus, say,
 * as zsw_fasta_parse_batch hands them back. The context's scoring applies to all of them; the panel is independent of
 * zsw_set_reference. With f = zsw_score_batch_from and R_k(i) = f(read_i) with r_k as the reference, the panel result of read i is
 * R_k(i) of the member k that ranks highest — ZSW_STATUS_OVERFLOWED > ZSW_STATUS_SOME by score > ZSW_STATUS_UNMAPPED =
 * ZSW_STATUS_EMPTY, as for the strands; ties go to the LOWEST k. out_ref[i] = that k; it is 0 for a read that is UNMAPPED or EMPTY
 * against every member. Score, status and tier are bit for bit what f returns against r_k, for every input, on every run,
 * whatever order the device work happens in.
 * The library does not score every read against every member: k-mers of the read looked up in each member's index
 * bound what the read can score against that member at all, the most promising member is scored first, and another member only if
 * its bound does not already rank it below (or level, from a higher k). Same results for every input; ZSW_OPTION_EXACT_PRUNING = 0,
 * or a matrix the index cannot serve, scores every read against every member.
 * Not covered: zsw_group_*, the shared-profile role, panel forms of the ends, ranges, direct (one <T, N>) and alignment calls (take
 * the group of a member with zsw_panel_gather_batch, zsw_set_reference that member and use any entry point on the group), strand
 * and panel in one call, ZSW_OPTION_MIN_SCORE, ZSW_ENCODING_PACKED4. */

/* The panel: member k is seqs[offsets[k] .. offsets[k + 1]) — exactly the `sequences` / `seq_offsets` arrays of
 * zsw_fasta_parse_batch. Both arrays lie in host or in device memory (`mem`); device arrays are taken where they lie, as
 * zsw_set_reference(.., ZSW_MEM_DEVICE) takes a reference. Errors: n_refs of 0 or above ZSW_PANEL_MAX_REFS and offsets that are
 * not ascending (ZSW_ERR_INVALID_ARGUMENT), a member of length 0 (ZSW_ERR_EMPTY_SEQUENCE); the panel set before stays as it is.
 * The context keeps a device copy and a host copy of the members and an index per member, built with the first panel call that can
 * use it and rebuilt after zsw_set_scoring; everything is released in zsw_destroy. Replacing a panel synchronises the device. */
zsw_error zsw_set_panel(zsw_context* ctx, const uint8_t* seqs, const uint64_t* offsets /* n_refs + 1 */, uint32_t n_refs, zsw_mem mem);

/* zsw_score_batch_from under the contract above; out_tier is optional, out_ref is not. Host and device batches, fixed and ragged,
 * ZSW_ENCODING_BYTES; ZSW_ENCODING_PACKED4 returns ZSW_ERR_UNSUPPORTED, and so does the call while ZSW_OPTION_MIN_SCORE is on.
 * ZSW_ERR_NOT_CONFIGURED if no panel or no scoring is set. n_refs = 1 is the plain call with out_ref all 0.
 * The call synchronises the stream twice: for the sizes of the groups of the first round (the reads by their first-choice member)
 * and for the lengths of the lists of the second round (per member, the reads it still has to be scored for) — and, like every
 * call, once more for a ragged device batch, whose size comes back from the device, and once per scored group of such a batch,
 * whose longest read does. Device workspace: 2 * n_refs + 13 bytes per read, a compact copy of the largest group and its results
 * (9 bytes per read) — for a host batch also the staged batch itself and its results; kept by the context until zsw_destroy.
 * A host batch crosses PCIe whole, in one copy, before the first kernel, and stays on the device for both rounds.
 * After the call zsw_prune_rescored reports on the last score pass the call ran, as after a strand-aware call. */
zsw_error zsw_score_panel_batch_from(zsw_context* ctx, const zsw_batch* reads, int from_width, int preset_bits, uint32_t* out_score,
                                     uint8_t* out_status, uint8_t* out_tier, uint32_t* out_ref, void* stream);

/* The panel's zsw_orient_batch: the reads with ref_of[i] == k, in input order, as a batch of the input's layout — out_bases, and
 * for a ragged batch out_offsets (*out_n + 1 entries; NULL for a fixed-length batch); out_index[j] = the input read the j-th
 * output read is, *out_n their number. The output arrays are the caller's, as large as the input's (out_index: one entry per read),
 * and live where reads->mem says, as ref_of does; a device batch is processed on the device (one synchronisation, for *out_n), a
 * host batch on the host. Needs neither scoring nor panel. ZSW_ENCODING_PACKED4 returns ZSW_ERR_UNSUPPORTED. With it any entry
 * point (3-pass, ranges, annotate, pile-up) runs per member: zsw_set_reference on member k, then the call on the group of k. */
zsw_error zsw_panel_gather_batch(zsw_context* ctx, const zsw_batch* reads, const uint32_t* ref_of, uint32_t k, uint8_t* out_bases,
                                 uint64_t* out_offsets, uint32_t* out_index, uint64_t* out_n, void* stream);

/* Counters of the context's last panel score call: out[0] reads settled after one score (every other member was ruled out by
 * proof; with n_refs = 1 every read), out[1] (read, member) pairs scored in the first round = the reads of the call, out[2] pairs
 * scored in the second round, out[3] reads scored against every member. No device work: the call itself has read them. */
zsw_error zsw_panel_counts(zsw_context* ctx, uint64_t* out /* 4 entries */);

/* ---- shared profile: one profile, many sequences ------------------------------------------- */
/* The other role of the striped functions (sw/mod.rs:63-67: "the profile can be aligned against any number of different
 * sequences"; SharedProfiles, profile_set.rs:552-560; Nucleotides::into_shared_profile, nucleotides/mod.rs:295-299): the
 * profile is built ONCE from a sequence the context holds — typically the reference — and read i is the sequence
 * sw_simd_* walks row by row. Scores are the numbers of the entry points above; ends, ranges and CIGARs are not in tie
 * cases, because the tie rule (first row, then first column) and the striping <T, N, nv = ceil(len / N)> now run over the
 * other sequence. In the results `ref_*` is the non-profile sequence, i.e. the READ, and `query_*` the profile sequence, as
 * sw_simd_* return them; invert != 0 is SeqSrc::Query(read_i) (alignment/mod.rs:176-190), which hands the roles back.
 *
 * zsw_set_profile_sequence: StripedProfile::new's sequence argument; len == 0 -> ZSW_ERR_EMPTY_SEQUENCE (profile.rs:32-44).
 * An empty READ is an empty `reference` argument here: status ZSW_STATUS_UNMAPPED (striped.rs:219-221).
 * Reads of up to 6,800 bases; the alignment calls keep plen x (longest read) flag bytes per read in flight.
 * With ZSW_OPTION_EXACT_PRUNING (the default) the score calls, and the first pass of the ends / ranges / alignment calls, take the
 * seeded exact pass with the roles swapped (an index of the profile sequence under the transposed matrix, built with the first
 * such call): a read whose maximum sits in exactly one cell of its matrix has the same ends under either tie rule; every other
 * read is computed over all its cells under this role's own rule. Same results either way. */
zsw_error zsw_set_profile_sequence(zsw_context* ctx, const uint8_t* sequence, size_t len, zsw_mem mem);
/* StripedProfile::<int_type,lanes,S>::new(sequence).sw_score(read_i) / ProfileSets::sw_score_from_i{from_width} */
zsw_error zsw_score_shared_batch(zsw_context* ctx, const zsw_batch* reads, zsw_int_type int_type, int lanes, uint32_t* out_score,
                                 uint8_t* out_status, void* stream);
zsw_error zsw_score_shared_batch_from(zsw_context* ctx, const zsw_batch* reads, int from_width, int preset_bits, uint32_t* out_score,
                                      uint8_t* out_status, uint8_t* out_tier, void* stream);
/* sw_simd_score_ends(reference = read_i, profile of the sequence): out_ref_end = exclusive end in the READ, out_query_end =
 * exclusive end in the profile sequence; first read position holding the maximum, then the first sequence position. */
zsw_error zsw_score_ends_shared_batch(zsw_context* ctx, const zsw_batch* reads, zsw_int_type int_type, int lanes, uint32_t* out_score,
                                      uint32_t* out_ref_end, uint32_t* out_query_end, uint8_t* out_status, void* stream);
/* sw_simd_score_ranges / ProfileSets::sw_score_ranges_from_i{from_width}: ref range = in the read, query range = in the sequence */
zsw_error zsw_score_ranges_shared_batch(zsw_context* ctx, const zsw_batch* reads, zsw_int_type int_type, int lanes, uint32_t* out_score,
                                        uint32_t* out_ref_start, uint32_t* out_ref_end, uint32_t* out_query_start, uint32_t* out_query_end,
                                        uint8_t* out_status, void* stream);
zsw_error zsw_score_ranges_shared_batch_from(zsw_context* ctx, const zsw_batch* reads, int from_width, int preset_bits, uint32_t* out_score,
                                             uint32_t* out_ref_start, uint32_t* out_ref_end, uint32_t* out_query_start, uint32_t* out_query_end,
                                             uint8_t* out_status, uint8_t* out_tier, void* stream);
/* sw_simd_align / ProfileSets::sw_align_from_i{from_width} with the shared profile; invert = 1 is the usual call,
 * `sequence.into_shared_profile(..).sw_align_from_i8(SeqSrc::Query(read_i))`. Outputs as zsw_align_batch(_from). */
zsw_error zsw_align_shared_batch(zsw_context* ctx, const zsw_batch* reads, zsw_int_type int_type, int lanes, int invert, zsw_alignment* out_aln,
                                 uint8_t* out_status, uint32_t* out_inc, uint8_t* out_op, uint64_t ciglet_cap, uint64_t* out_n_ciglets,
                                 void* stream);
zsw_error zsw_align_shared_batch_from(zsw_context* ctx, const zsw_batch* reads, int from_width, int preset_bits, int invert,
                                      zsw_alignment* out_aln, uint8_t* out_status, uint8_t* out_tier, uint32_t* out_inc, uint8_t* out_op,
                                      uint64_t ciglet_cap, uint64_t* out_n_ciglets, void* stream);
/* StripedProfile::sw_align_3pass / ProfileSets::sw_align_from_i{from_width}_3pass with the shared profile (profile.rs:536-552,
 * profile_set.rs:212-283, 552-560 -> three_pass.rs:21-104): the shared role's ranges, then sw_banded_align / sw_scalar_align over
 * the bounding box with the roles of three_pass.rs (`reference` = read i, ScalarProfile over the profile sequence's sub-range) —
 * the form the reference documents for a large reference and small queries. Like the reference's, the CIGAR may differ from
 * zsw_align_shared_batch's where several optimal alignments exist. invert = 1: SeqSrc::Query(read_i). Outputs as zsw_align_batch(_from). */
zsw_error zsw_align_3pass_shared_batch(zsw_context* ctx, const zsw_batch* reads, zsw_int_type int_type, int lanes, int invert, zsw_alignment* out_aln,
                                       uint8_t* out_status, uint32_t* out_inc, uint8_t* out_op, uint64_t ciglet_cap, uint64_t* out_n_ciglets,
                                       void* stream);
zsw_error zsw_align_3pass_shared_batch_from(zsw_context* ctx, const zsw_batch* reads, int from_width, int preset_bits, int invert,
                                            zsw_alignment* out_aln, uint8_t* out_status, uint8_t* out_tier, uint32_t* out_inc, uint8_t* out_op,
                                            uint64_t ciglet_cap, uint64_t* out_n_ciglets, void* stream);

/* ---- annotation of alignments: =/X CIGARs, edit counts, path score ------------------------------- */
/* One pass over the records an alignment call wrote (or any caller-built records), beside the two sequences each was aligned
 * between. Per read with status[i] == ZSW_STATUS_SOME the library builds the Alignment of the record, with ref_in_alignment = the
 * record's reference sequence [ref_start, ref_end), and computes
 *   path_score / path_status  sw_score_from_path (src/alignment/sw/mod.rs:399-454) statement for statement: ops M = X I D S N H P,
 *                             gap_open + gap_extend * (inc - 1) per I / D ciglet, the first error in that function's own order
 *                             (ZSW_PATH_* 1..6 mirror ScoringError);
 *   the counts                columns under M, = and X are compared and counted as matches or mismatches; I / D ciglets add to the
 *                             base and run counts; S N H P count nothing (NM = mismatches + ins_bases + del_bases);
 *   the verbose CIGAR         (if out_aln is given) AlignmentStates::to_verbose_sequence_matching(reference, query, ref_start)
 *                             (src/alignment/types/state.rs:320-342; Alignment::to_verbose_sequence_matching, types/output.rs:456-479):
 *                             each M column becomes = or X through add_state, every other ciglet goes through add_ciglet, so equal
 *                             neighbours merge (3=2M whose M starts with two matches gives 5=) and no ciglet has inc == 0.
 * flags say which call produced the records:
 *   zsw_align*_batch(_from), and the *_strands_* 3-pass call on the oriented batch of zsw_orient_batch:
 *                                      invert == 0: 0                                     invert != 0: ZSW_ANNOTATE_READ_IS_REF
 *   zsw_align*_shared_batch(_from):    invert == 0: ZSW_ANNOTATE_SHARED | ZSW_ANNOTATE_READ_IS_REF    invert != 0: ZSW_ANNOTATE_SHARED
 * ZSW_ANNOTATE_READ_IS_REF: ref_* of a record index the read and query_* the context's sequence (without it the other way round).
 * ZSW_ANNOTATE_SHARED: the other sequence is the one of zsw_set_profile_sequence and the read takes the matrix's row axis
 * (weights[idx(read) * S + idx(seq)]); without it the other sequence is the one of zsw_set_reference and the read takes the column
 * axis (weights[idx(ref) * S + idx(read)]): row = non-profile residue, column = profile residue, whatever invert was.
 * ZSW_ANNOTATE_MATCH_RESIDUES: a column is a match when index_map sends both bytes to the same residue; by default raw bytes are
 * compared, which is the reference's rule (state.rs:330): `a` against `A` is X.
 * aln / status: n_reads entries; inc / op: n_ciglets pairs; every array lives where reads->mem says. out_stats: n_reads
 * zsw_alignment_stats (declared void*: a zsw_alignment_stats array converts without a cast).
 * out_aln[i] = aln[i] with n_ciglets / ciglet_offset pointing into out_inc / out_op, the reads laid out in read order (no atomics
 * decide a place: the output is the same on every run). Capacity protocol of the alignment calls: *out_n_ciglets receives the
 * total; beyond ciglet_cap the call returns ZSW_ERR_INVALID_ARGUMENT with the required size there (the stats are written all the same).
 * Reads that are not walked — zeroed stats but for path_status, out_aln[i] copied with no ciglets —: status[i] != ZSW_STATUS_SOME
 * (ZSW_PATH_NO_ALIGNMENT); ciglets that leave [0, n_ciglets), ref_start > ref_end, a range or length that disagrees with the actual
 * sequences, an inc of 0, a merged inc beyond 32 bits (ZSW_PATH_BAD_RECORD); an op outside MIDNSHP=X (ZSW_PATH_INVALID_CIGAR_OP); and
 * a path that leaves a sequence (ZSW_PATH_REFERENCE_ENDED, ZSW_PATH_QUERY_ENDED: the reference's conversion would panic there).
 * ZSW_PATH_FULL_*_NOT_USED and ZSW_PATH_NEGATIVE_SCORE keep counts and verbose CIGAR. Records and ciglets are caller memory: every
 * index derived from them is checked in 64-bit arithmetic before the load that uses it; a malformed record is a status, never a fault.
 * Without out_aln the call is asynchronous for device batches; with it, it synchronises once for the total. Host batches are staged
 * and the call is synchronous. ZSW_ENCODING_PACKED4: ZSW_ERR_UNSUPPORTED. Output arrays must not overlap inputs or each other;
 * unknown flag bits or a null required pointer: ZSW_ERR_INVALID_ARGUMENT; scoring, or the sequence the flags name, not set:
 * ZSW_ERR_NOT_CONFIGURED. Lanes per alignment and the LDS threshold of the context's sequence: zoe_amd/csrc/zsw_annotate.hpp. */
typedef struct zsw_alignment_stats { /* 32 bytes */
    uint32_t matches, mismatches;    /* columns under M, = or X, by the chosen equality */
    uint32_t ins_bases, del_bases;   /* sum of inc over I / D ciglets */
    uint32_t ins_runs, del_runs;     /* number of I / D ciglets */
    int32_t path_score;              /* sw_score_from_path; the negative sum for ZSW_PATH_NEGATIVE_SCORE; else 0 */
    uint32_t path_status;            /* zsw_path_status */
} zsw_alignment_stats;
typedef enum zsw_path_status {
    ZSW_PATH_OK = 0, ZSW_PATH_REFERENCE_ENDED = 1, ZSW_PATH_QUERY_ENDED = 2, ZSW_PATH_FULL_QUERY_NOT_USED = 3,
    ZSW_PATH_FULL_REFERENCE_NOT_USED = 4, ZSW_PATH_INVALID_CIGAR_OP = 5, ZSW_PATH_NEGATIVE_SCORE = 6, ZSW_PATH_NO_ALIGNMENT = 7,
    ZSW_PATH_BAD_RECORD = 8
} zsw_path_status;
enum { ZSW_ANNOTATE_READ_IS_REF = 1, ZSW_ANNOTATE_SHARED = 2, ZSW_ANNOTATE_MATCH_RESIDUES = 4 };
zsw_error zsw_annotate_batch(zsw_context* ctx, const zsw_batch* reads, int flags, const zsw_alignment* aln, const uint8_t* status,
                             const uint32_t* inc, const uint8_t* op, uint64_t n_ciglets, void* out_stats,
                             zsw_alignment* out_aln, uint32_t* out_inc, uint8_t* out_op, uint64_t ciglet_cap, uint64_t* out_n_ciglets,
                             void* stream);

/* ---- SAM records formatted on the device ------------------------------------------------------------ */
/* The text SamData::from_alignment (src/data/records/sam/mod.rs:223-245) followed by Display for SamData
 * (records/sam/std_traits.rs:3-44) print for every read of a batch, in read order, one line per read, each closed by '\n':
 *   status[i] == ZSW_STATUS_SOME:  QNAME FLAG RNAME POS MAPQ CIGAR * 0 0 SEQ QUAL AS:i:score [NM:i:nm]
 *   any other status:              QNAME 4    *     0   0    *     * 0 0 SEQ QUAL
 * tab-separated. FLAG is 0, or 16 where strand[i] != 0; POS = ref_start + 1; CIGAR is the decimal inc and the op byte of each of the
 * record's ciglets in order, `*` for a record without ciglets (Display for Cigar, cigar/mod.rs:146-158); NM = mismatches + ins_bases
 * + del_bases of stats[i], appended where `stats` is given. POS and NM are 64-bit sums. SEQ is the read's bytes as they stand in
 * `reads` — for the records of a strand-aware call that is the oriented batch of zsw_orient_batch, as for zsw_annotate_batch —, QUAL
 * its quality bytes, back to front where strand[i] != 0; a read of length 0 has `*` for both (is_missing_sam_field, sam/mod.rs:425-428).
 * No byte of a name, a base or a quality is looked at or escaped. The @HD / @SQ header is the caller's.
 * The call formats whatever records it is given — those of an alignment call, or out_aln / out_inc / out_op of zsw_annotate_batch (the
 * = / X CIGAR) — and reads neither reference nor scoring: a context is all it needs (ctx == NULL: ZSW_ERR_NOT_CONFIGURED). Records
 * are caller memory. A ZSW_STATUS_SOME record whose ciglets leave [0, n_ciglets) (64-bit, checked before any ciglet load), or with an
 * inc of 0 or an op outside MIDNSHP=X, is written as an unmapped line and counted in *out_n_bad: a count, never a fault. For device
 * arrays a name (or a read) whose end offset lies in front of its start has length 0; host offsets, of the reads or of the names,
 * that go backwards are ZSW_ERR_INVALID_ARGUMENT.
 * Capacity protocol of the alignment calls: *out_n_bytes always receives the total; beyond text_cap the call returns
 * ZSW_ERR_INVALID_ARGUMENT having written out_line_offsets and no byte of out_text; out_text == NULL with text_cap == 0 is the
 * sizing call (ZSW_OK; the length launch and the scan only). No byte at or beyond out_text[total] is written. out_line_offsets
 * (optional, n_reads + 1 entries): line i = out_text[off[i], off[i + 1]). Every array lives where reads->mem says, but for
 * fields->rname, out_n_bytes and out_n_bad (host). Three steps — a length launch, an exclusive sum, a write launch — with no atomic
 * deciding a place: the text is the same on every run. Host batches are staged and the call is synchronous; device batches
 * synchronise the stream once, for the total and the count. Workspace, kept by the context until zsw_destroy: 17 bytes per read, and
 * the staged arrays and the text of a host batch.
 * Unknown flag bits, mapq > 255, rname_len outside 1..255, a null required pointer (reads, fields, rname, aln, status, out_n_bytes,
 * out_n_bad; bases unless ZSW_SAM_OMIT_SEQ with quals == NULL; inc / op with n_ciglets; qname_offsets with qnames), or an output array
 * that overlaps an input or the other output: ZSW_ERR_INVALID_ARGUMENT, nothing written. ZSW_ENCODING_PACKED4: ZSW_ERR_UNSUPPORTED.
 * ZSW_OPTION_MIN_SCORE and ZSW_OPTION_EXACT_PRUNING do not matter here (a ZSW_STATUS_BELOW_MIN_SCORE read is an unmapped line);
 * zsw_group_* does not cover the call. Lanes per line, lines per block and the LDS cap of a line: zoe_amd/csrc/zsw_sam.hpp. */
typedef struct zsw_sam_fields {        /* zero-initialise; every device/host array lives where reads->mem says */
    const uint8_t*  qnames;            /* QNAME bytes of all reads, back to back; NULL: every QNAME is "*" */
    const uint64_t* qname_offsets;     /* n_reads + 1 entries; name i = qnames[off[i], off[i+1]) */
    const uint8_t*  quals;             /* laid out exactly as reads->bases (fixed_len or reads->offsets); NULL: QUAL "*" */
    const uint8_t*  strand;            /* optional, n_reads: != 0 -> FLAG 16 and QUAL written back to front */
    const void*     stats;             /* optional, n_reads zsw_alignment_stats: appends NM:i: to mapped lines */
    const char*     rname;             /* HOST memory always; rname_len bytes, 1..255 */
    uint32_t        rname_len;
    uint32_t        mapq;              /* 0..255, written on mapped lines (the driver uses 255) */
} zsw_sam_fields;
enum { ZSW_SAM_OMIT_SEQ = 1 };         /* SEQ "*" on every line (with quals == NULL the text carries no per-base bytes) */
/* fields: a zsw_sam_fields (declared const void*, as out_stats above: a zsw_sam_fields* converts without a cast) */
zsw_error zsw_sam_batch(zsw_context* ctx, const zsw_batch* reads, const void* fields, int flags, const zsw_alignment* aln,
                        const uint8_t* status, const uint32_t* inc, const uint8_t* op, uint64_t n_ciglets, uint8_t* out_text,
                        uint64_t text_cap, uint64_t* out_n_bytes, uint64_t* out_line_offsets /* optional, n_reads + 1 */,
                        uint64_t* out_n_bad, void* stream);

/* ---- pile-up: per-site base counts and the plurality consensus ------------------------------------ */
/* zsw_pileup_batch reduces the records of an alignment call to one table over the context's sequence, the one the reads were
 * aligned to: counts[pos].bin[b] = how often a byte of bin b stood opposite position pos. What AlignmentComposition::per_site_counts
 * (src/composition/by_position/mod.rs:248-287) gives over the query rows of pairwise_align_with (src/alignment/pairwise.rs:26-65),
 * placed at the positions of the reference row. The eight bins, in the order of NucleotideCounts::into_inner():
 *   0 `A a`   1 `C c`   2 `G g`   3 `T t U u`   4 `N n`   5 `-`   6 the other IUPAC letters R Y S W K M B D H V in either case and `.`
 *   7 every other byte.  The bins do not depend on the context's index_map.
 * flags: ZSW_ANNOTATE_READ_IS_REF and ZSW_ANNOTATE_SHARED with the meaning they have for zsw_annotate_batch (which sequence the
 * record's ref_* index, and which of the context's two sequences is meant; the table above says which call needs which), and
 * ZSW_PILEUP_CLEAR. ZSW_ANNOTATE_MATCH_RESIDUES is not accepted. The record's reference cursor starts at ref_start, its query cursor
 * at 0; S moves the query cursor, H and P do nothing.
 *   without READ_IS_REF (record reference = the sequence, record query = the read):
 *     M = X   counts[pos].bin[bin(read byte)] += 1 for each of the inc columns
 *     D       counts[pos].bin[5] += 1 for each of the inc positions
 *     N       counts[pos].bin[4] += 1 for each of the inc positions (the reference writes literal N bytes there)
 *     I       no site count; ins[p].runs += 1 and ins[p].bases += inc with p the reference cursor: the insertion lies in front of
 *             position p, p in 0..=len
 *   with READ_IS_REF (record query = the sequence, record reference = the read) the gap ops change places: I is the gap bin at
 *     inc positions, D goes to ins[] at the query cursor, N counts nothing and moves the read cursor, S skips positions of the
 *     sequence without counting them, columns count bin(read byte) at the query cursor's position.
 * Positions the ciglets do not cover get nothing. len = the length of the sequence the flags name; counts: len zsw_site_counts;
 * ins: optional, len + 1 zsw_site_insertions (both declared void*, as out_stats of zsw_annotate_batch: the arrays convert without
 * a cast). The call ADDS to both tables, so batches accumulate; ZSW_PILEUP_CLEAR zeroes them first. The counters are 32-bit and
 * wrap: a site covered by more than 2^32 - 1 reads is the caller's concern. All arithmetic is modulo 2^32 and addition commutes:
 * the table is the same on every run.
 * All or nothing: a read contributes only if status[i] == ZSW_STATUS_SOME and its record passes the checks of zsw_annotate_batch
 * that need no base: the ciglets inside [0, n_ciglets), ranges and lengths that agree with the actual sequences, no inc of 0, no
 * op outside MIDNSHP=X, and no ciglet that leaves either sequence (the reference's within [ref_start, ref_end)). Every other
 * ZSW_STATUS_SOME record contributes nothing at all and is counted in *out_n_bad (host memory). The ciglets are validated in a pass
 * of their own before a counter is touched, and every index derived from caller memory is checked in 64-bit arithmetic before
 * the load or add that uses it: a malformed record is a count, never a fault.
 * Every array lives where reads->mem says, except out_n_bad. Device batches synchronise the stream once, for *out_n_bad. Host
 * batches are staged and the call is synchronous: the host tables are copied in, added to and copied back. n_reads == 0 is ZSW_OK
 * and, without ZSW_PILEUP_CLEAR, leaves the tables as they were. Unknown flag bits, a null required pointer (reads, out_n_bad,
 * counts; bases, aln, status with reads; inc / op with n_ciglets), or a table that overlaps an input or the other table:
 * ZSW_ERR_INVALID_ARGUMENT, nothing written. The sequence the flags name not set: ZSW_ERR_NOT_CONFIGURED (scoring is not needed).
 * ZSW_ENCODING_PACKED4, or a sequence of 2^31 - 1 bases or more: ZSW_ERR_UNSUPPORTED.
 * Workspace, kept by the context until zsw_destroy: 16 bytes per position of the sequence (three difference arrays and the per-site
 * mismatches, see zoe_amd/csrc/zsw_pileup.hpp, which also has the lanes per alignment, the alignments per block and the sequence
 * length up to which a block accumulates in LDS), the scan's scratch, and the staged arrays and tables of a host batch.
 * zsw_group_* does not cover the call: the sum across GPUs is one all-reduce of the table and is left to the caller.
 *
 * zsw_consensus_from_counts: out_seq[pos] = NucleotideCounts::plurality_acgtn (by_position/mod.rs:147-162) of counts[pos]: the
 * largest of bins 0..4, ties in the order A > C > G > T > N by strict >, so a site without any such count is `A`; the gap bin never
 * wins. With ZSW_CONSENSUS_KEEP_UNCOVERED a site whose bins 0..4 are all zero takes fallback[pos] instead (what a refinement loop
 * wants for the uncovered ends). counts, fallback and out_seq live where `mem` says; a device call is asynchronous on `stream`, a
 * host call is staged and synchronous. out_seq in device memory is a valid argument of zsw_set_reference(.., ZSW_MEM_DEVICE): a
 * refinement round never leaves the card. Needs neither scoring nor a sequence. Unknown flag bits, a null required pointer, or
 * out_seq over an input: ZSW_ERR_INVALID_ARGUMENT; len == 0: ZSW_OK. */
typedef struct zsw_site_counts { uint32_t bin[8]; } zsw_site_counts;             /* NucleotideCounts<u32> */
typedef struct zsw_site_insertions { uint32_t runs, bases; } zsw_site_insertions;
enum { ZSW_PILEUP_CLEAR = 8 };             /* beside the ZSW_ANNOTATE_* role bits */
zsw_error zsw_pileup_batch(zsw_context* ctx, const zsw_batch* reads, int flags, const zsw_alignment* aln, const uint8_t* status,
                           const uint32_t* inc, const uint8_t* op, uint64_t n_ciglets, void* counts /* len zsw_site_counts */,
                           void* ins /* optional, len + 1 zsw_site_insertions */, uint64_t* out_n_bad /* host */, void* stream);
enum { ZSW_CONSENSUS_KEEP_UNCOVERED = 1 };
zsw_error zsw_consensus_from_counts(zsw_context* ctx, const void* counts, uint64_t len, zsw_mem mem, int flags,
                                    const uint8_t* fallback /* len bytes, with KEEP_UNCOVERED */, uint8_t* out_seq /* len */,
                                    void* stream);

/* ---- FASTQ parsed on the device --------------------------------------------------------------------- */
/* zsw_fastq_parse_batch turns a buffer of single-line FASTQ into the arrays zsw_batch and zsw_sam_fields take: the bases of all
 * records back to back with out_offsets, the qualities laid out the same way, the names back to back with out_qname_offsets. The
 * semantics are FastQReader's (src/data/records/fastq/reader.rs:87-187). A line ends at '\n'; only the last line of the buffer can be
 * unterminated; record r is lines 4 r .. 4 r + 3. With ZSW_FASTQ_FINAL the buffer ends the file: a non-empty unterminated tail is a
 * line, the records are ceil(lines / 4), and a line the file does not have reads as empty. Without it only the records whose four
 * lines are all terminated are parsed; the tail is neither parsed nor an error (the caller prepends it to the next chunk).
 * chop_line_break removes one trailing '\n' and then one trailing '\r'; a '\r' without a '\n' behind it stays. Per record, the first
 * failing check, in the reader's order, is its code:
 *   1 ZSW_FASTQ_MISSING_AT        the header line does not start with '@' (a blank line where a header belongs, too)
 *   2 ZSW_FASTQ_MISSING_HEADER    nothing behind '@' after the chop
 *   3 ZSW_FASTQ_INVALID_UTF8      the header is not UTF-8 by String::from_utf8: overlong forms, surrogates, values above U+10FFFF
 *                                 and truncated sequences are invalid
 *   4 ZSW_FASTQ_MISSING_SEQUENCE  the sequence line is empty after the chop
 *   5 ZSW_FASTQ_MISSING_PLUS      the third line does not start with '+' (the rest of that line is ignored)
 *   6 ZSW_FASTQ_MISSING_QUALITY   the quality line is empty after the chop
 *   7 ZSW_FASTQ_LENGTH_MISMATCH   sequence and quality differ in length
 *   8 ZSW_FASTQ_INVALID_QUALITY   a quality byte outside '!' ..= '~'
 * Trailing blank lines are not skipped. The records in front of the failing record with the lowest index are delivered — what a
 * consumer of the iterator that stops at the first Err has seen; that index is a minimum over the records, not an order of arrival,
 * and outputs and report are the same on every run. The name is the whole header behind '@', chopped; with ZSW_FASTQ_NAME_TO_BLANK
 * it ends in front of the first space or tab (what zsw_driver writes as QNAME). The UTF-8 check always covers the whole header.
 * Positions and lengths are 64-bit throughout.
 * text and every output array live where `mem` says; out_info is host memory, ZSW_FASTQ_INFO_WORDS entries, always filled by a call
 * that gets past its argument checks: RECORDS delivered, their BASES and NAME_BYTES, CONSUMED = the offset one past the last delivered
 * record (a caller that reads a file in chunks restarts there), ERROR = 0 or a code of the table with ERROR_RECORD the failing
 * record's index and ERROR_OFFSET the start of its header line (both 0 without an error), MIN_LEN / MAX_LEN over the delivered
 * sequences (0 for none; where they are equal the bases are a fixed-length batch as well). A malformed file is ZSW_OK and a report,
 * never a fault: every position derived from the text is checked in 64-bit arithmetic before the load that uses it. n_bytes == 0 is
 * ZSW_OK with zero records. out_offsets and out_qname_offsets hold record_cap + 1 entries. out_quals, or out_qnames together with
 * out_qname_offsets, may be NULL: that part is not written (and name_cap is ignored, NAME_BYTES still reported).
 * Capacity protocol, as for zsw_sam_batch: RECORDS > record_cap, BASES > base_cap or NAME_BYTES > name_cap is
 * ZSW_ERR_INVALID_ARGUMENT with the needed sizes in out_info and no byte of any output array written; every output NULL with every
 * capacity 0 is the sizing call (ZSW_OK). Bounds that always suffice, so that a caller can do without the sizing call:
 *   base_cap = n_bytes / 2,  name_cap = n_bytes,  record_cap = n_bytes / 8 + 1  (the shortest record is "@x\nA\n+\nA" at the file's end)
 * No byte at or beyond out_bases[BASES], out_quals[BASES], out_qnames[NAME_BYTES] or entry RECORDS + 1 of the offsets is written.
 * Unknown flag bits, a null required pointer (ctx, out_info; text with n_bytes > 0; out_bases and out_offsets outside the sizing
 * call; one of out_qnames / out_qname_offsets without the other), an unknown mem, or an output that overlaps the text or another
 * output: ZSW_ERR_INVALID_ARGUMENT, nothing written, out_info included. More than 2^36 bytes, or about 2^33 newlines, per call: ZSW_ERR_UNSUPPORTED.
 * The launches: newlines counted per tile, an exclusive sum, the position of every newline at its rank, a record pass (one wavefront
 * per record), two exclusive sums for the offsets, a gather; a minimum and a maximum are the only atomics. Device calls synchronise the
 * stream once, for the report; one case aside: the workspace for the newline positions is sized for a newline per 16 bytes before the
 * count is known, and a denser text makes the call repeat its later launches once with the exact size. Host calls are staged and
 * synchronous. The call needs neither scoring nor a reference, ZSW_OPTION_* do not matter, and zsw_group_* does not cover it.
 * Workspace, kept by the context until zsw_destroy: 8 bytes per newline (n_bytes / 2 at least), 33 bytes per four newlines, 16 bytes
 * per tile, the scans' scratch, and the staged text and outputs of a host call. Tile and block constants: zoe_amd/csrc/zsw_fastq.hpp. */
enum { ZSW_FASTQ_FINAL = 1, ZSW_FASTQ_NAME_TO_BLANK = 2 };
enum { ZSW_FASTQ_MISSING_AT = 1, ZSW_FASTQ_MISSING_HEADER = 2, ZSW_FASTQ_INVALID_UTF8 = 3, ZSW_FASTQ_MISSING_SEQUENCE = 4,
       ZSW_FASTQ_MISSING_PLUS = 5, ZSW_FASTQ_MISSING_QUALITY = 6, ZSW_FASTQ_LENGTH_MISMATCH = 7, ZSW_FASTQ_INVALID_QUALITY = 8 };
enum { ZSW_FASTQ_INFO_RECORDS = 0, ZSW_FASTQ_INFO_BASES = 1, ZSW_FASTQ_INFO_NAME_BYTES = 2, ZSW_FASTQ_INFO_CONSUMED = 3,
       ZSW_FASTQ_INFO_ERROR = 4, ZSW_FASTQ_INFO_ERROR_RECORD = 5, ZSW_FASTQ_INFO_ERROR_OFFSET = 6,
       ZSW_FASTQ_INFO_MIN_LEN = 7, ZSW_FASTQ_INFO_MAX_LEN = 8, ZSW_FASTQ_INFO_WORDS = 9 };
zsw_error zsw_fastq_parse_batch(zsw_context* ctx, const uint8_t* text, uint64_t n_bytes, zsw_mem mem, int flags, uint8_t* out_bases,
                                uint8_t* out_quals, uint64_t base_cap, uint64_t* out_offsets, uint8_t* out_qnames, uint64_t name_cap,
                                uint64_t* out_qname_offsets, uint64_t record_cap, uint64_t* out_info, void* stream);

/* ---- FASTA parsed on the device --------------------------------------------------------------------- */
/* zsw_fasta_parse_batch turns a buffer of FASTA into the arrays zsw_batch and zsw_sam_fields take, and into sequences that
 * zsw_set_reference(.., ZSW_MEM_DEVICE) takes where they lie: the sequences of all records back to back with out_offsets, the names
 * back to back with out_name_offsets. There are no qualities (zsw_sam_fields.quals == NULL prints QUAL '*'). The semantics are
 * FastaReader's (src/data/records/fasta/mod.rs:241-410), restated on the positions of the buffer's '>' bytes:
 *   Start of the file. Lines end at '\n'. Lines that hold nothing but ASCII whitespace (space, \t, \n, \x0c, \r; not \x0b), an
 *   unterminated last one too, are skipped; the first other line must have '>' as its first byte, else MISSING_GT; a text without
 *   such a line is NO_DATA.
 *   Records. EVERY '>' byte delimits: the region of a record runs from behind its '>' to the next '>' anywhere, or to the end.
 *   Header of the file's first record: to the end of its line, then chop_line_break (one '\n', then one '\r'; a '\r' elsewhere in
 *   it stays in the name). Empty after the chop: MISSING_HEADER; a '>' in that line: GT_IN_HEADER.
 *   Header of every later record: it ends in front of the first '\n' OR '\r' of the region, so a lone '\r' ends it and what follows
 *   is sequence. Empty, or the text ends right behind the '>': MISSING_HEADER. No line break in a region that ends at '>' (">>"
 *   too): GT_IN_HEADER; none in one that ends the text: MISSING_SEQUENCE.
 *   Sequence: the rest of the region with every '\n' and every '\r' removed, wherever they stand; every other byte stays (blanks,
 *   lower case, '\0', bytes >= 0x80). Empty: MISSING_SEQUENCE — with one exception the reader has: a later record that ends at
 *   '>' and whose region holds no '\n' at all (">b\r>c") is GT_IN_HEADER. Not empty, and the region ends at a '>' whose preceding
 *   byte is not '\n' ("\r>" too): GT_IN_SEQUENCE.
 *   1 ZSW_FASTA_NO_DATA   2 ZSW_FASTA_MISSING_GT   3 ZSW_FASTA_MISSING_HEADER   4 ZSW_FASTA_GT_IN_HEADER
 *   5 ZSW_FASTA_MISSING_SEQUENCE   6 ZSW_FASTA_GT_IN_SEQUENCE
 * Names are the raw header bytes: the reader makes a String of them with from_utf8_lossy, so no byte is an error, and nothing is
 * replaced here. With ZSW_FASTA_NAME_TO_BLANK a name ends in front of its first space or tab; the emptiness check covers the whole
 * header.
 * ZSW_FASTA_FINAL: the buffer ends the file. Without it the record that starts at the last '>' of the buffer is neither parsed nor
 * an error and CONSUMED is the offset of that '>'; a buffer without '>' that is all whitespace consumes its terminated lines;
 * NO_DATA is not reported; MISSING_GT is, as soon as a byte that is not whitespace stands in front of the first '>' at a line
 * start; and every error that a following '>' proves is reported as with FINAL.
 * ZSW_FASTA_CONTINUED: the buffer starts at the '>' of a record that is not the file's first — what a caller that restarts at
 * CONSUMED passes. The start-of-file rules do not apply and record 0 takes the later-record header rule. A first byte other than
 * '>' (an empty buffer too): ZSW_ERR_INVALID_ARGUMENT, no output written.
 * Taken unchanged from zsw_fastq_parse_batch: the meaning of the nine report words — RECORDS delivered, their BASES and
 * NAME_BYTES, CONSUMED = the offset one past the last delivered record (the '>' of the first record not delivered, or n_bytes),
 * ERROR = 0 or a code with ERROR_RECORD the failing record's index and ERROR_OFFSET the offset of its '>', MIN_LEN / MAX_LEN over
 * the delivered sequences —; here NO_DATA and MISSING_GT concern record 0, leave CONSUMED 0, and ERROR_OFFSET is 0 for NO_DATA and
 * the first byte that is not whitespace for MISSING_GT. The records in front of the failing record with the lowest index are
 * delivered; that index is a minimum, not an order of arrival; no atomic decides a place, a minimum and a maximum are the only
 * atomics, and outputs and report are identical on every run. A malformed text is ZSW_OK and a report, never a fault: every
 * position taken from memory is clamped into the text, in 64-bit arithmetic, before a load uses it. n_bytes == 0 is ZSW_OK with zero
 * records (NO_DATA with FINAL). text and every output array live where `mem` says, at any byte address; out_info is host memory,
 * ZSW_FASTA_INFO_WORDS entries. out_offsets and out_name_offsets hold record_cap + 1 entries. out_names together with
 * out_name_offsets may be NULL: names are not written (name_cap is ignored, NAME_BYTES still reported).
 * Capacity protocol: RECORDS > record_cap, BASES > base_cap or NAME_BYTES > name_cap is ZSW_ERR_INVALID_ARGUMENT with the needed
 * sizes in out_info and no byte of any output array written; every output NULL with every capacity 0 is the sizing call (ZSW_OK).
 * Bounds that always suffice, so that a caller can do without the sizing call:
 *   base_cap = n_bytes,  name_cap = n_bytes,  record_cap = n_bytes / 4 + 1  (the shortest record is ">a\nA" at the file's end)
 * No byte at or beyond out_bases[BASES], out_names[NAME_BYTES] or entry RECORDS + 1 of the offsets is written.
 * Unknown flag bits, a null required pointer (ctx, out_info; text with n_bytes > 0; out_bases and out_offsets outside the sizing
 * call; one of out_names / out_name_offsets without the other), an unknown mem, or an output that overlaps the text or another
 * output: ZSW_ERR_INVALID_ARGUMENT, nothing written, out_info included. More than 2^36 bytes, or about 2^31 '>', per call:
 * ZSW_ERR_UNSUPPORTED.
 * The launches — none does work that grows with the length of one record, so ten million short records and one wrapped chromosome
 * cost the same per byte: the index of zsw_fastq_parse_batch made over '>' (count per tile, exclusive sum, position at rank); a
 * record pass (one wavefront per record: the header, the line breaks that open the body, every code); an exclusive sum for the name
 * offsets; the sequence pass over tiles of the text (kept bytes per tile, exclusive sum, every kept byte written at its rank, the
 * lane that meets a '>' writes that record's offset); a gather for the names. Device calls synchronise the stream once, for the
 * report; one case aside: the workspace for the '>' positions is sized for one per 64 bytes before the count is known, and a denser
 * text makes the call repeat its later launches once with the exact size. Host calls are staged and synchronous. The call needs
 * neither scoring nor a reference, ZSW_OPTION_* do not matter, and zsw_group_* does not cover it. Workspace, kept by the context
 * until zsw_destroy: 41 bytes per '>' (for one '>' per 64 bytes of text at least), 32 bytes per tile, the scans' scratch, and the staged text and
 * outputs of a host call. Tile and block constants: zoe_amd/csrc/zsw_text.hpp, zsw_fasta.hpp. */
enum { ZSW_FASTA_FINAL = 1, ZSW_FASTA_NAME_TO_BLANK = 2, ZSW_FASTA_CONTINUED = 4 };
enum { ZSW_FASTA_NO_DATA = 1, ZSW_FASTA_MISSING_GT = 2, ZSW_FASTA_MISSING_HEADER = 3, ZSW_FASTA_GT_IN_HEADER = 4,
       ZSW_FASTA_MISSING_SEQUENCE = 5, ZSW_FASTA_GT_IN_SEQUENCE = 6 };
enum { ZSW_FASTA_INFO_RECORDS = 0, ZSW_FASTA_INFO_BASES = 1, ZSW_FASTA_INFO_NAME_BYTES = 2, ZSW_FASTA_INFO_CONSUMED = 3,
       ZSW_FASTA_INFO_ERROR = 4, ZSW_FASTA_INFO_ERROR_RECORD = 5, ZSW_FASTA_INFO_ERROR_OFFSET = 6,
       ZSW_FASTA_INFO_MIN_LEN = 7, ZSW_FASTA_INFO_MAX_LEN = 8, ZSW_FASTA_INFO_WORDS = 9 };
zsw_error zsw_fasta_parse_batch(zsw_context* ctx, const uint8_t* text, uint64_t n_bytes, zsw_mem mem, int flags, uint8_t* out_bases,
                                uint64_t base_cap, uint64_t* out_offsets, uint8_t* out_names, uint64_t name_cap,
                                uint64_t* out_name_offsets, uint64_t record_cap, uint64_t* out_info, void* stream);

/* ---- SAM parsed on the device ----------------------------------------------------------------------- */
/* zsw_sam_parse_batch turns a buffer of SAM text into the arrays zsw_annotate_batch, zsw_sam_batch, zsw_pileup_batch and (through
 * the pile-up) zsw_consensus_from_counts take: per data line a zsw_alignment with its status and its ciglets in inc / op, and the
 * reads as bases / quals / qnames with offsets, as zsw_fastq_parse_batch leaves them. Lines and fields are SAMReader's
 * (src/data/records/sam/reader.rs:189-286), records SamData::is_unmapped / to_alignment's (sam/mod.rs:305-354), ciglets as
 * AlignmentStates::try_from(&Cigar) builds them (src/alignment/types/std_traits.rs:119-155).
 * Lines (BufRead::lines): a line ends at '\n'; one '\n' and then one '\r' in front of it are removed, a bare trailing '\r' stays.
 * With ZSW_SAMTEXT_FINAL a non-empty unterminated tail is a line; without it the tail is neither parsed nor an error and CONSUMED
 * says where the caller restarts. Nothing behind the last '\n' is a line. A line that starts with '@' is a header line: counted
 * and skipped, wherever it stands. A blank line is a data line with one field.
 * Reader errors: per line the first failing check, in this order, is the line's code, and delivery ends in front of the line with
 * the lowest index that has one — what a consumer who stops at the first Err has seen; a minimum over the lines, not an order of
 * arrival:
 *   1 ZSW_SAMTEXT_INVALID_UTF8     the line is not UTF-8 by String::from_utf8 (header lines too)
 *   2 ZSW_SAMTEXT_TOO_FEW_FIELDS   fewer than 11 tab-separated fields
 *   3 ZSW_SAMTEXT_INVALID_FLAG     | str::parse::<u16 / usize / u8>: one optional '+', then at least one ASCII digit and nothing
 *   4 ZSW_SAMTEXT_INVALID_POS      | else; leading zeros are allowed; the value must be within the type (usize is 64-bit); "-0",
 *   5 ZSW_SAMTEXT_INVALID_MAPQ     | "+", an empty field and a blank inside the field are errors
 *   6 ZSW_SAMTEXT_INVALID_QUALITY  QUAL is neither empty nor "*" and holds a byte outside '!' ..= '~'
 * RNEXT, PNEXT and TLEN are not looked at. The CIGAR is not validated by the reader: it is trim_ascii-ed, and "*" is the empty CIGAR.
 * Score: what opt_fields.get("AS") followed by .int() gives (sam/mod.rs:517-540, 581-633). The optional fields are taken in order; a
 * field without a ':' in front of the AS field is an Err; the first field whose tag text is "AS" decides: its type must be the single
 * character 'i' and its value must parse as i64 (optional '+' / '-', then digits). Ok(Some(v)) with 0 <= v <= 2^32 - 1 is the score;
 * everything else is score 0 and ZSW_SAMREC_BIT_NO_SCORE.
 * Conversion, for every delivered data line i, into status[i], aln[i] and the ciglets:
 *  1. Unmapped iff FLAG & 4, or the sum of inc over the M D N = X ciglets that the UNCHECKED CigletIterator yields is 0
 *     (cigar/iter.rs:52-99: left to right; it stops silently at the first byte that is neither digit nor op, at an op without digits,
 *     or at an inc beyond 64 bits; it yields incs of 0 and ignores trailing digits — "0M", "5I3Q" and "Q" are unmapped with code 0):
 *     ZSW_STATUS_UNMAPPED and a zeroed record.
 *  2. With `rname` given, a line whose RNAME differs from it byte for byte: ZSW_STATUS_UNMAPPED, a zeroed record and
 *     ZSW_SAMREC_BIT_OTHER_RNAME; no conversion is attempted (the context has one reference; files name several).
 *  3. Otherwise the record is converted; the first code in this order makes it ZSW_STATUS_UNMAPPED, zeroed, with the code in
 *     parsed[i].code, and counts it in CODED:
 *       1 ZSW_SAMREC_SEQ_MISSING           SEQ is empty or "*"
 *       2 ZSW_SAMREC_CIGAR_INVALID_OP      | the first error of CigletIteratorChecked (iter.rs:478-537): a byte that is neither
 *       3 ZSW_SAMREC_CIGAR_MISSING_INC     | digit nor one of MIDNSHPX=, an op without digits, an inc of 0, an inc beyond 64 bits,
 *       4 ZSW_SAMREC_CIGAR_INC_ZERO        | digits without an op behind them
 *       5 ZSW_SAMREC_CIGAR_INC_OVERFLOW    |
 *       6 ZSW_SAMREC_CIGAR_MISSING_OP      |
 *       7 ZSW_SAMREC_CIGAR_MERGE_OVERFLOW  the merged inc of adjacent equal ops leaves 64 bits
 *       8 ZSW_SAMREC_POS_ZERO              pos - 1 would underflow
 *       9 ZSW_SAMREC_CLIPS_EXCEED_SEQ      query_len - soft_clipping would underflow
 *      10 ZSW_SAMREC_TOO_LARGE             a merged inc, pos - 1 + ref_len_in_alignment, the number of ciglets or the length of SEQ
 *                                          does not fit the 32-bit fields of zsw_alignment (all sums 64-bit and saturating)
 *     Where the reference returns Err or panics on a record with two of these faults, which of the two it names may differ from this
 *     order (it subtracts pos - 1 and the clips before it validates the CIGAR, and meets a merge overflow before a later ciglet's
 *     error). Neither side ever delivers such a record as an alignment.
 *  4. A converted record is ZSW_STATUS_SOME with score from AS, ref_start = pos - 1, ref_end = ref_start + ref_len_in_alignment,
 *     ref_len = the call's argument, query_len = the length of SEQ. The soft clips are taken from the RAW ciglets, before merging:
 *     from the front one optional H and then one optional S; from the back the same, among the ciglets the front has not consumed
 *     ("2S3S5M" clips 2 in front); query_start = front, query_end = front + (query_len - front - back). The ciglets are the
 *     checked ciglets with adjacent equal ops merged ("3M2M" is 5M; no inc is 0), laid out in record order: ciglet_offset /
 *     n_ciglets point into inc / op, and no atomic decides a place. As in the reference, SEQ's length is not compared with the
 *     CIGAR's query length: zsw_annotate_batch and zsw_pileup_batch report such records as bad.
 * Reads: SEQ bytes go to bases as they stand (a missing SEQ is a read of length 0 with ZSW_SAMREC_BIT_SEQ_MISSING), QNAME bytes to
 * qnames, QUAL to quals in the layout of bases. A QUAL that is missing, or whose length differs from SEQ's, fills its slot with '!'
 * and sets ZSW_SAMREC_BIT_QUAL_MISSING or ZSW_SAMREC_BIT_QUAL_LENGTH (the reference accepts both kinds of line). With
 * ZSW_SAMTEXT_QUAL_FORWARD the QUAL of a record with FLAG & 16 is stored back to front: (bases, quals, strand) is then what
 * zsw_sam_fields expects, and zsw_sam_batch -> zsw_sam_parse_batch -> zsw_sam_batch gives the same bytes.
 * out: a zsw_sam_parse_out (declared const void*, as `fields` of zsw_sam_batch). text and every array of it live where `mem` says;
 * rname and out_info are host memory. out_info holds ZSW_SAMTEXT_INFO_WORDS entries, always filled by a call that gets past its
 * argument checks: RECORDS (data lines delivered), HEADERS (header lines in front of CONSUMED), BASES, NAME_BYTES, CIGLETS, CONSUMED
 * (the offset one past the last delivered line), ERROR = 0 or a reader code with ERROR_LINE the failing line's index among all lines
 * and ERROR_OFFSET its first byte (both 0 without an error), MAPPED (records with status SOME), CODED, MIN_LEN / MAX_LEN over the
 * delivered reads. A malformed file is ZSW_OK and a report, never a fault: every position derived from the text is checked in 64-bit
 * arithmetic before the load that uses it. n_bytes == 0 is ZSW_OK with nothing delivered.
 * Capacity protocol, as for zsw_fastq_parse_batch: RECORDS > record_cap, BASES > base_cap, NAME_BYTES > name_cap or CIGLETS >
 * ciglet_cap is ZSW_ERR_INVALID_ARGUMENT with the needed sizes in out_info and no byte of any output written; every output NULL with
 * every capacity 0 is the sizing call (ZSW_OK). Bounds that always suffice, so that a caller can do without the sizing call:
 *   base_cap = n_bytes,  name_cap = n_bytes,  ciglet_cap = n_bytes / 2,  record_cap = n_bytes / 14 + 1
 * (the shortest data line is ten tabs and three digits). quals, qnames together with qname_offsets, strand and parsed may be NULL:
 * that part is not written (NAME_BYTES is still reported). Unknown flag bits, a null required pointer (ctx, out, out_info; text with
 * n_bytes > 0; bases, offsets, aln, status, inc, op outside the sizing call; one of qnames / qname_offsets or of rname / rname_len
 * without the other), rname_len > 255, an unknown mem, or an output that overlaps the text or another output:
 * ZSW_ERR_INVALID_ARGUMENT, nothing written, out_info included. More than 2^36 bytes or 2^31 lines per call: ZSW_ERR_UNSUPPORTED.
 * The launches: the newline index of zsw_fastq_parse_batch, a line pass (one wavefront per line), six exclusive sums over the
 * delivered lines, a gather that walks each CIGAR once more to write its ciglets; a minimum and a min / max are the only atomics and
 * the outputs are the same on every run. Device calls synchronise the stream once, for the report; the workspace for the newline
 * positions is sized for a line per 64 bytes before the count is known, and a denser text makes the call repeat its later launches
 * once with the exact size. Host calls are staged and synchronous. The call needs neither scoring nor a reference, ZSW_OPTION_* do
 * not matter, and zsw_group_* does not cover it. Workspace, kept by the context until zsw_destroy: 8 bytes per newline, 176 bytes
 * per line (n_bytes * 2.75 at least), 16 bytes per tile, the scans' scratch, and the staged text and outputs of a host call. */
typedef struct zsw_sam_parsed {        /* 24 bytes, one per delivered record */
    uint64_t pos;                      /* POS as parsed (1-based; 0 allowed on unmapped lines) */
    uint64_t line;                     /* index of the record's line among ALL lines of the text, headers included */
    uint16_t flag;                     /* FLAG */
    uint8_t  mapq;                     /* MAPQ */
    uint8_t  code;                     /* 0, or a ZSW_SAMREC_* conversion code */
    uint32_t bits;                     /* ZSW_SAMREC_BIT_* */
} zsw_sam_parsed;
typedef struct zsw_sam_parse_out {     /* zero-initialise; every array lives where `mem` says; caps in entries */
    uint8_t*  bases;    uint8_t* quals;          /* quals optional; laid out exactly as bases */
    uint64_t  base_cap; uint64_t* offsets;       /* record_cap + 1 */
    uint8_t*  qnames;   uint64_t name_cap; uint64_t* qname_offsets; /* both or neither; record_cap + 1 */
    zsw_alignment* aln; uint8_t* status;         /* record_cap each */
    uint32_t* inc;      uint8_t* op; uint64_t ciglet_cap;
    uint8_t*  strand;                            /* optional, record_cap: (FLAG & 16) != 0 */
    void*     parsed;                            /* optional, record_cap zsw_sam_parsed */
    uint64_t  record_cap;
} zsw_sam_parse_out;
enum { ZSW_SAMTEXT_FINAL = 1, ZSW_SAMTEXT_QUAL_FORWARD = 2 };
enum { ZSW_SAMTEXT_INVALID_UTF8 = 1, ZSW_SAMTEXT_TOO_FEW_FIELDS = 2, ZSW_SAMTEXT_INVALID_FLAG = 3, ZSW_SAMTEXT_INVALID_POS = 4,
       ZSW_SAMTEXT_INVALID_MAPQ = 5, ZSW_SAMTEXT_INVALID_QUALITY = 6 };
enum { ZSW_SAMREC_SEQ_MISSING = 1, ZSW_SAMREC_CIGAR_INVALID_OP = 2, ZSW_SAMREC_CIGAR_MISSING_INC = 3, ZSW_SAMREC_CIGAR_INC_ZERO = 4,
       ZSW_SAMREC_CIGAR_INC_OVERFLOW = 5, ZSW_SAMREC_CIGAR_MISSING_OP = 6, ZSW_SAMREC_CIGAR_MERGE_OVERFLOW = 7, ZSW_SAMREC_POS_ZERO = 8,
       ZSW_SAMREC_CLIPS_EXCEED_SEQ = 9, ZSW_SAMREC_TOO_LARGE = 10 };
enum { ZSW_SAMREC_BIT_NO_SCORE = 1, ZSW_SAMREC_BIT_OTHER_RNAME = 2, ZSW_SAMREC_BIT_SEQ_MISSING = 4, ZSW_SAMREC_BIT_QUAL_MISSING = 8,
       ZSW_SAMREC_BIT_QUAL_LENGTH = 16 };
enum { ZSW_SAMTEXT_INFO_RECORDS = 0, ZSW_SAMTEXT_INFO_HEADERS = 1, ZSW_SAMTEXT_INFO_BASES = 2, ZSW_SAMTEXT_INFO_NAME_BYTES = 3,
       ZSW_SAMTEXT_INFO_CIGLETS = 4, ZSW_SAMTEXT_INFO_CONSUMED = 5, ZSW_SAMTEXT_INFO_ERROR = 6, ZSW_SAMTEXT_INFO_ERROR_LINE = 7,
       ZSW_SAMTEXT_INFO_ERROR_OFFSET = 8, ZSW_SAMTEXT_INFO_MAPPED = 9, ZSW_SAMTEXT_INFO_CODED = 10, ZSW_SAMTEXT_INFO_MIN_LEN = 11,
       ZSW_SAMTEXT_INFO_MAX_LEN = 12, ZSW_SAMTEXT_INFO_WORDS = 13 };
zsw_error zsw_sam_parse_batch(zsw_context* ctx, const uint8_t* text, uint64_t n_bytes, zsw_mem mem, int flags,
                              const char* rname /* HOST, optional */, uint32_t rname_len, uint32_t ref_len,
                              const void* out /* zsw_sam_parse_out */, uint64_t* out_info /* host */, void* stream);

/* ---- pre-alignment filter ------------------------------------------------------------------ */
/* out_pass[i] = sneaky_snake(&reference[ref_start[i] .. ref_start[i]+ref_len[i]], read_i, threshold)
 * (src/alignment/sneaky_snake.rs:78-131): the SneakySnake edit-distance filter between a read and a candidate window of the
 * context's reference; `threshold` is the allowed edits as a fraction of the read length. Bytes are compared raw, as in the
 * reference (no index map). ref_start / ref_len / out_pass live where `reads->mem` says. A window that leaves the reference
 * is ZSW_ERR_INVALID_ARGUMENT for host arrays and ZSW_FILTER_BAD_WINDOW in out_pass for device arrays.
 * reads->encoding must be ZSW_ENCODING_BYTES, in host and in device memory: packed residue indices are not the bytes the filter
 * compares, so ZSW_ENCODING_PACKED4 (and any unknown value) is ZSW_ERR_INVALID_ARGUMENT before anything is copied. Host offsets
 * that go backwards are ZSW_ERR_INVALID_ARGUMENT, as in the scoring calls. */
typedef enum zsw_filter_result {
    ZSW_FILTER_REJECT = 0,      /* Some(false) */
    ZSW_FILTER_PASS = 1,        /* Some(true)  */
    ZSW_FILTER_NONE = 2,        /* None: threshold outside [0,1] or |len difference| > allowed edits */
    ZSW_FILTER_BAD_WINDOW = 255
} zsw_filter_result;
zsw_error zsw_sneaky_snake_batch(zsw_context* ctx, const zsw_batch* reads, const uint32_t* ref_start, const uint32_t* ref_len,
                                 float threshold, uint8_t* out_pass, void* stream);

/* ---- several GPUs behind one handle --------------------------------------------------------- */
/* The batched counterpart of scoring many reads against SharedProfiles (src/alignment/profile_set.rs:552-560) from many
 * threads: one caller, one batch, n GPUs. Reads shard into contiguous index ranges [i*n/G, (i+1)*n/G), context i takes shard i
 * on device_ids[i] from its own host thread; scoring tables and reference are replicated; nothing is exchanged while the
 * kernels run. A device may be listed more than once (two contexts on one GPU). A group is used from one host thread at a time;
 * the contexts it owns are reachable through zsw_group_context (e.g. for zsw_timing_* or to run other entry points per shard). */
typedef struct zsw_group zsw_group;
zsw_error zsw_group_create(const int* device_ids, int n_devices, zsw_group** out);
void zsw_group_destroy(zsw_group* group);
int zsw_group_size(const zsw_group* group);
zsw_context* zsw_group_context(zsw_group* group, int i);
const char* zsw_group_last_error_string(const zsw_group* group);
zsw_error zsw_group_set_scoring(zsw_group* group, const int8_t* weights, int S, const uint8_t* index_map, int gap_open,
                                int gap_extend);
zsw_error zsw_group_set_reference(zsw_group* group, const uint8_t* reference, size_t len); /* host memory */

/* ProfileSets::sw_score_from_i{from_width} (src/alignment/profile_set.rs:71-107) for every read of a batch in HOST memory,
 * spread over the group's GPUs. out_score / out_status / out_tier (optional) are host arrays of reads->n_reads entries and are
 * written in place, shard by shard: no collective is involved. Synchronous. */
zsw_error zsw_group_score_batch_from(zsw_group* group, const zsw_batch* reads, int from_width, int preset_bits,
                                     uint32_t* out_score, uint8_t* out_status, uint8_t* out_tier);

/* ProfileSets::sw_align_from_i{from_width} (src/alignment/profile_set.rs:124-179) and sw_align_from_i{from_width}_3pass
 * (:212-283) for a batch in HOST memory spread over the group's GPUs; arguments as in zsw_align_batch_from /
 * zsw_align_3pass_batch_from. The shards are aligned in parallel; records, statuses and tiers land in read order and the
 * ciglets of the shards are laid out one after the other (ciglet_offset indexes the caller's arrays). If ciglet_cap is too
 * small the call returns ZSW_ERR_INVALID_ARGUMENT with the required size in *out_n_ciglets. Synchronous. */
zsw_error zsw_group_align_batch_from(zsw_group* group, const zsw_batch* reads, int from_width, int preset_bits, int invert,
                                     zsw_alignment* out_aln, uint8_t* out_status, uint8_t* out_tier, uint32_t* out_inc,
                                     uint8_t* out_op, uint64_t ciglet_cap, uint64_t* out_n_ciglets);
zsw_error zsw_group_align_3pass_batch_from(zsw_group* group, const zsw_batch* reads, int from_width, int preset_bits, int invert,
                                           zsw_alignment* out_aln, uint8_t* out_status, uint8_t* out_tier, uint32_t* out_inc,
                                           uint8_t* out_op, uint64_t ciglet_cap, uint64_t* out_n_ciglets);

/* zsw_group_score_batch_from with reads and results in DEVICE memory: shards[i] is the batch of context i on device_ids[i]; out_score[i] and
 * out_status[i] are arrays on device i with room for ALL reads (sum of the shards' n_reads). Context i writes its slice in
 * place and one RCCL all-gather over xGMI (grouped broadcasts: the shards need not be equal) completes the arrays on every
 * device, in shard order. librccl is opened at the first call; without it the call returns ZSW_ERR_UNSUPPORTED. Synchronous. */
zsw_error zsw_group_score_batch_from_device(zsw_group* group, const zsw_batch* shards, int from_width, int preset_bits,
                                            uint32_t* const* out_score, uint8_t* const* out_status);

/* ---- bench/test utilities (not part of the reference surface) ------------------------------ */
/* Counter-based synthetic reads: read i depends only on (seed, i, reference), so any
 * shard regenerates its own slice. Writes reads [first, first+n) of length `len` into out (device). */
zsw_error zsw_synth_reads(zsw_context* ctx, uint64_t seed, uint64_t first, uint64_t n, uint32_t len, uint8_t* out_device,
                          void* stream);
/* Ragged variant: lengths uniform in [min_len, max_len]; offsets_device[n+1] must hold the exclusive
 * prefix sum of zsw_synth_length(seed, first+i, ..) (see zoe_amd/synth.py). */
zsw_error zsw_synth_reads_ragged(zsw_context* ctx, uint64_t seed, uint64_t first, uint64_t n, uint32_t min_len,
                                 uint32_t max_len, const uint64_t* offsets_device, uint8_t* out_device, void* stream);
uint32_t zsw_synth_length(uint64_t seed, uint64_t index, uint32_t min_len, uint32_t max_len);

/* Runs a small on-device check of the instruction-level assumptions the kernels make (v_perm byte
 * order, cross-lane shuffle direction, packed saturation). Returns ZSW_OK or ZSW_ERR_HIP with the
 * failing check named in zsw_last_error_string. */
zsw_error zsw_selftest(zsw_context* ctx);

/* Host twins of the generator (no GPU needed): tests and the CPU baseline consume the same bytes. */
void zsw_synth_reference_host(uint64_t seed, uint64_t len, uint8_t* out);
void zsw_synth_reads_host(uint64_t seed, uint64_t first, uint64_t n, uint32_t len, const uint8_t* ref, uint32_t R,
                          uint8_t* out);
void zsw_synth_reads_ragged_host(uint64_t seed, uint64_t first, uint64_t n, uint32_t min_len, uint32_t max_len,
                                 const uint64_t* offsets, const uint8_t* ref, uint32_t R, uint8_t* out);

/* HIP-event timing of the kernels of each *_batch call (its whole first pass for score calls), recorded on the call's stream.
 * zsw_timing_read synchronises on the recorded events, returns the summed kernel seconds and the
 * number of launches since the last read, and resets. For bench.py's roofline line. */
zsw_error zsw_timing_enable(zsw_context* ctx, int enable);
zsw_error zsw_timing_read(zsw_context* ctx, double* seconds, uint64_t* launches);
/* The same for the one kernel that dominates a score call on the default path: seed_window_kernel of the seeded exact pass
 * (events around that launch alone, on its stream; a ragged batch has one launch per length class). 0 launches if the calls
 * since the last read took another path. For bench.py's roofline of that kernel. */
zsw_error zsw_timing_read_window(zsw_context* ctx, double* seconds, uint64_t* launches);

/* Options of a context. ZSW_OPTION_EXACT_PRUNING (value 0 / 1, default 1): the seeded exact first pass (zsw_score_seed.hip;
 * DESIGN.md 4.1e). sw_simd_score returns only the maximum of the DP matrix (striped.rs:65-142), so every entry point that starts
 * with a score pass (score, ends, ranges, alignment, 3-pass alignment) first looks a few k-mers of each read up in an index of
 * the reference, computes a band of diagonals around the one they agree on, and accepts the maximum found there only if upper bounds
 * show that no alignment elsewhere can reach it; every other read is scored over all its cells. Same results for every input;
 * roughly an order of magnitude fewer cells on reads that resemble the reference, the cost of the full pass plus a few per
 * cent on reads that do not. 28 bytes + 4 bits per base of device workspace per read, up to 0.3 GB of strip-boundary buffers per
 * call, and 8 * 4^K bytes of index (K = 8 for a 2 kb reference: 512 KiB; K = 10 for 30 kb: 8 MiB). Value 0 frees the workspace and computes every cell of every read.
 * Alphabets of 8..32 letters (amino-acid matrices: a substituted residue may cost as little as 1, which leaves the k-mer argument
 * nothing to prove with) take the column-pruned pass instead (zsw_score_prune.hip): the first 24 or 48 columns of
 * a read against every row of the reference, the other columns in a window of rows around the strip's best row, and bounds that
 * add each remaining column's own largest score; reads of 65..400 residues in batches of 98,304 or more, 8 bytes per read pair
 * and reference row of workspace for up to 2 M reads at a time; the first chip-full of a large batch decides whether the rest is
 * worth it (above 70 % handed back the others go straight to the full pass).
 *
 * ZSW_OPTION_MIN_SCORE (value T in [0, 2^31 - 1], default 0 = off: not one byte of any result changes). The caller discards
 * reads that score less than T anyway; with T > 0 the library says so instead of computing their score. Let (status, score, ...)
 * be what a covered call returns with T = 0 and thr the overflow threshold of the call's last width (255 / 65,535 / 2^32 - 1 for
 * signed types, T::MAX - bias for unsigned ones). A read that is ZSW_STATUS_UNMAPPED, or ZSW_STATUS_SOME with score <
 * min(T, thr), reports ZSW_STATUS_BELOW_MIN_SCORE with score 0, tier 0 (no width answered: which one would have is not known
 * without the score), ends / ranges 0 and, in alignment calls, a zeroed record without ciglets. Every other read — SOME with
 * score >= T, OVERFLOWED, EMPTY (decided by length before anything else) — is bit for bit what T = 0 returns, whichever kernel
 * settled it: min(T, thr) keeps a read of true score in [thr, T) OVERFLOWED on every route. Reads are settled below T by the
 * upper bounds the seeded pass computes anyway (the bound over the whole reference in the seed kernel, the bounds of a band
 * walk), which spares them the pass over all their cells, or else by their exact score.
 * Covered (read-as-profile role; host and device batches, fixed and ragged, both encodings): zsw_score_batch(_from),
 * zsw_score_ends_batch, zsw_score_ranges_batch(_from), zsw_align_3pass_batch(_from); in the ranges and 3-pass calls T applies to
 * the forward pass, and a read below T takes no reverse pass, bounding box or DP — as an UNMAPPED read. Alphabets of 8..32
 * letters get the contract from the exact score alone. Not covered: zsw_align_batch(_from) and every *_shared_* and *_strands_*
 * call return ZSW_ERR_UNSUPPORTED while T > 0 and write nothing. zsw_group_* (no option setter) and zsw_sneaky_snake_batch (no
 * score) are unaffected.
 * Unknown options or values return ZSW_ERR_INVALID_ARGUMENT. */
typedef enum zsw_option { ZSW_OPTION_EXACT_PRUNING = 1, ZSW_OPTION_MIN_SCORE = 2 } zsw_option;
zsw_error zsw_set_option(zsw_context* ctx, zsw_option option, int64_t value);

/* ZSW_OPTION_MIN_SCORE: how the context's last covered call settled the reads it reports as ZSW_STATUS_BELOW_MIN_SCORE (the forward
 * pass of a ranges / 3-pass call): out[0] by the bound over the whole reference in the seed kernel, out[1] by the bounds of a band
 * walk, out[2] by their exact score, out[3] all of them. All 0 while the option is off. Synchronises the device. With T > 0
 * zsw_prune_rescored goes down by the reads the bounds settle: it keeps counting the reads scored over all their cells. */
zsw_error zsw_min_score_counts(zsw_context* ctx, uint64_t* out /* 4 entries */);

/* Kernel-selection overrides for the parity tests (every path below is bit-identical to the default one; the tests
 * prove it by running both). Results never depend on these bits, only which kernel produces them. They are kept apart
 * from the options above: zsw_debug_set(ctx, 0) does not switch an option off. The library reads no environment variable. */
typedef enum zsw_debug_flag {
    ZSW_DEBUG_SCORE_V1 = 1,          /* score: Zoe's signed-offset arithmetic (score_kernel) instead of the drift-domain kernel */
    ZSW_DEBUG_NO_TILES = 2,          /* score: reads longer than the widest strip configuration go to the exact 32-bit kernel */
    ZSW_DEBUG_NO_W32 = 4,            /* score: scores beyond the packed range go to the exact 32-bit kernel, not the 32-bit tile kernel */
    ZSW_DEBUG_NO_WIDE = 8,           /* score: 8..32-letter alphabets go to the exact 32-bit kernel */
    ZSW_DEBUG_NO_SIDE_STREAMS = 16,  /* score: length classes of a ragged batch run one after the other */
    ZSW_DEBUG_NO_PIPELINE = 32,      /* score: host batches are copied whole before the kernel */
    ZSW_DEBUG_ALIGN_NO_PACKED = 64,  /* align: the 32-bit one-read-per-lane-group kernel answers every group */
    ZSW_DEBUG_SCORE_PRUNE = 128,     /* the bit ZSW_OPTION_EXACT_PRUNING holds (set by default); here for completeness */
    ZSW_DEBUG_SCORE_PRUNE_ANY_SIZE = 256, /* pruned passes for batches of every size (by default batches under 1,024 reads take the full pass) */
    /* with SCORE_PRUNE: round 2's column-pruned pass (zsw_score_prune.hip) instead of the seeded one: a narrow
     * strip of query columns against every reference row, the other columns in a window of rows around the strip's best row,
     * bound checks, the full pass for the reads that fail one. Reads of 65..400 bases, batches of 98,304 reads or more (or
     * ANY_SIZE), up to 32 GiB of workspace. A cross-check of the seeded pass for the 5-letter tables; the default first pass of
     * 8..32-letter alphabets (no flag needed there). */
    ZSW_DEBUG_PRUNE_STRIP = 512,
    /* align: the second pass starts warmup_rows before the first kept row for every read (round 2), not at the row the seeded
     * first pass certifies (zsw_seed.hpp: seed_safe_start) */
    ZSW_DEBUG_ALIGN_LONG_WARMUP = 1024,
    /* the seeded pass computes whole rows around the anchor (seed_window_kernel) instead of the band of diagonals of
     * seed_band_kernel (zsw_score_band.hip) */
    ZSW_DEBUG_SEED_NO_BAND = 2048,
    /* score: the banded kernel walks every read in the full band at once (no narrow first band for short reads) */
    ZSW_DEBUG_SEED_WIDE_BAND = 4096,
    /* score: reads the seeded pass hands back walk every row of a long reference as one item each (by default they are cut
     * into chunks of rows that run as independent items, zsw_score_v2.hpp: ScoreArgsV2::chunk_rows) */
    ZSW_DEBUG_NO_ROW_CHUNKS = 8192,
    /* score + ranges: the reverse pass of sw_simd_score_ranges by the exact prefix kernel for every read (by default a second seeded
     * pass over the reversed sequences settles the reads whose maximum sits in one cell, forward and reversed) */
    ZSW_DEBUG_RANGES_EXACT_REVERSE = 16384,
    /* align: every read with an alignment goes through the second pass (the literal striped recurrence). By default a read with
     * exactly one optimal alignment that is a gapless diagonal — both maxima in one cell each, the diagonal's weights add up to the
     * score, the score beyond what any path with an insertion and a deletion between the same corners can reach — gets that
     * alignment without it (tests/models/align_gapless_cert.cpp) */
    ZSW_DEBUG_ALIGN_NO_CERTIFICATE = 32768,
    /* score: the first of the banded pass's two tiers walks 16-column strips (seed_band_kernel) for every read length. By default
     * score-only batches of reads of up to 255 bases walk it diagonal by diagonal (seed_diag_kernel, zsw_score_band.hip) */
    ZSW_DEBUG_SEED_STRIP_FIRST_TIER = 65536,
    /* score: in the diagonal first tier every lane derives the k-mer column patterns of its own two reads. By default a batch of
     * reads of one length derives them once per wavefront and group of columns, on scalar registers (a ragged batch always takes
     * the per-lane form) */
    ZSW_DEBUG_SEED_DIAG_LANE_EVENTS = 131072,
    /* score: the full pass over the reads the seed kernel hands back runs as launches of its own behind the band tiers. By default a
     * score-only call of two band tiers with reads of up to 152 bases (and no ZSW_OPTION_MIN_SCORE) scores them in the first tier's
     * launch: the hand-back blocks and the tier's persistent blocks share one grid (zsw_score_band.hip: seed_diag_handback_kernel) */
    ZSW_DEBUG_SEED_NO_COSCHEDULE = 262144,
    /* score: contiguous reads of one length of up to 160 bases are seeded by the one-pass kernel (seed_kernel<true, .>: every
     * thread sweeps its read byte by byte from LDS). By default the block converts its reads to packed rows once and every thread
     * sweeps words (zsw_score_seed.hip: seed_packed_kernel) */
    ZSW_DEBUG_SEED_PLAIN_KERNEL = 524288,
    /* score: the diagonal first tier walks every wavefront's reads with the edge masks applied and the sixteenth diagonal computed.
     * By default a wavefront of a one-length batch whose walks all stay inside the reference (zsw_seed_diag.hpp:
     * diag_walk_is_interior) takes a copy of the column loop without the masks, and a wavefront whose lane partners all share
     * their anchor skips the sixteenth diagonal's cell */
    ZSW_DEBUG_SEED_DIAG_MASKED = 1048576,
    /* score: the whole list the seed kernel hands back is scored in the first tier's launch. By default a one-length call of
     * 2,097,152 reads or more whose list is longer than a round of that launch (98,304 reads) and a slice cuts the last 16,384
     * reads off it, which run as a launch of score_kernel_v2 on a side stream beside the second tier (zsw_handback.hpp:
     * handback_slices) */
    ZSW_DEBUG_SEED_NO_SLICES = 2097152,
    /* score: slices at any batch size, for the tests: the last 128 reads of the list (if it has as many), and up to 128 reads in
     * front of them as a second slice beside the sort (zsw_handback.hpp: HANDBACK_TINY_*) */
    ZSW_DEBUG_SEED_TINY_SLICES = 4194304
} zsw_debug_flag;
zsw_error zsw_debug_set(zsw_context* ctx, uint32_t flags);

/* Tests only (tests/test_gpu_bounds.py): the banded seeded pass (zsw_score_band.hip) writes, for every read it walks, the
 * values its decision rests on into records[8 * read]: [0] the band's maximum (doubled; odd = held by a path through a cell
 * outside the band), [1] / [2] the most a path that ends above / below the band can score, [3] / [4] the smaller / larger anchor
 * diagonal of the lane's two reads, [5] strips | rows above the anchor << 8 | below << 20, [6] the read's own anchor diagonal,
 * [7] 1 = accepted by this walk | columns per strip << 8. A later tier overwrites an earlier one. The host model (tests/models/seed_band.cpp) computes
 * the same quantities from the read and this geometry; the test requires equality. records: device memory for 8 int32 per read
 * of the following calls, NULL = off (the default). */
zsw_error zsw_debug_band_records(zsw_context* ctx, int32_t* records);

/* Tests only (tests/test_gpu_cert.py): the certificate pass of the alignment calls (zsw_threepass.hip, classify and sweep launches;
 * the decision is zoe_amd/csrc/zsw_cert.hpp) writes, for every read with an alignment, four int32 into records[4 * read]:
 * [0] the verdict class — 0 a maximum not in one cell, 1 gapless certified, 2 one gap certified, 3 rejected: the diagonal does not
 * add up to the score, 4 rejected: the potential does not rule out three or more gap runs (one gap: or fewer than two pairs, or
 * gap_extend == 0), 5 rejected: an alignment with two gap runs reaches the score, 6 rejected: no single or adjacent set of one-run
 * placements reaches exactly the score, 7 deferred to the sweep launch (final only if that launch did not run) —; [1] the deciding
 * parameter — class 1: the run lengths k swept; 2 and 6: the last best placement (pairs before the run); 5: the first run's signed
 * length (a deletion counts +); 3: the diagonal's sum —; [2] one gap (2 and 6): the placements that reach the best score;
 * [3] 1 = decided by the sweep launch. Reads without an alignment and calls outside certificate mode leave their records alone.
 * records: device memory for 4 int32 per read of the following calls, NULL = off (the default). Results do not change. */
zsw_error zsw_debug_cert_records(zsw_context* ctx, int32_t* records);

/* Tests only (tests/test_gpu_threepass_edges.py): the third pass of the 3-pass alignment calls of both roles (zsw_threepass.hip)
 * writes, for every read with an alignment, eight int32 into records[8 * read]: [0] the route — 1 the no-gaps shortcut, 2 a banded
 * attempt was accepted, 3 the scalar alignment of the whole box —; [1] the band width of the accepted attempt, else 0; [2] the banded
 * attempts made by the launch that finished the read; [3] that launch — 0 classify, 1 the first DP launch, 2 the rerun with
 * full-size resources —; [4] why the first DP launch handed the read to the rerun — 0 it did not, 1 the two DP rows alone exceed
 * its slot, 2 a banded attempt did not fit, 3 the scalar alignment of the box did not fit, 4 more ciglets than that launch keeps
 * per read —; [5] reason 2: the band that did not fit, else 0; [6] the bytes of a slot of the launch that finished the read, 0 for
 * classify; [7] the ciglets written in traceback order. Reads without an alignment and the certificate mode of the zsw_align calls
 * leave their records alone. records: device memory for 8 int32 per read of the following calls, NULL = off (the default).
 * Results do not change. */
zsw_error zsw_debug_threepass_records(zsw_context* ctx, int32_t* records);

/* Tests only (tests/test_gpu_strands.py): the strand-aware calls (zsw_strand.hip) write, for every read, eight int32 into
 * records[8 * read]: [0] / [1] the support of the anchor vote on the forward / reverse strand, [2] / [3] the whole-reference bound
 * of the forward / reverse strand (no local alignment of that orientation scores more; -1: no bound), [4] the strand that ran
 * first, [5] 1 = settled by proof (the other strand was not scored), [6], [7] 0. The host model (tests/models/strand_bound.cpp)
 * computes [0..4] from the read; the test requires equality. Without a usable index: 0, 0, -1, -1, 0. records: device memory for
 * 8 int32 per read of the following calls, NULL = off (the default). Results do not change. */
zsw_error zsw_debug_strand_records(zsw_context* ctx, int32_t* records);

/* Tests only (tests/test_gpu_panel.py): zsw_score_panel_batch_from (zsw_panel.hip) writes, for every read, 2 + 2 * n_refs int32 into
 * records[(2 + 2 * n_refs) * read]: [0] the first-choice member (the largest support of the anchor vote, ties to the lowest member),
 * [1] 1 = settled after one score (every other member ruled out by proof), else 0, [2 .. 2 + n_refs) the supports of the anchor
 * vote per member, [2 + n_refs .. 2 + 2 * n_refs) the whole-reference bounds per member (no local alignment of the read against
 * that member scores more; -1: no bound). The host model (tests/models/panel_bound.cpp) computes all but [1] from the read, and [1]
 * from the score against the first choice; the test requires equality. Without a usable index: first choice 0, supports 0, bounds
 * -1. records: device memory for 2 + 2 * n_refs int32 per read of the following calls, NULL = off (the default). Results do not
 * change. */
zsw_error zsw_debug_panel_records(zsw_context* ctx, int32_t* records);

/* Tests only (tests/test_gpu_strip_edges.py): which score kernels the context's last call launched. The score launchers
 * (launch_score and launch_score_rev, zsw_score.hip) note every kernel launch they issue in a host-side list that is emptied
 * when a call stages its batch; no device work, no synchronisation, results do not change. A record is four uint32:
 * (kind, G, C, mode) — kind is a zsw_launch_kind, (G, C) the strip configuration the kernel was instantiated for (lanes per read
 * pair, columns per lane; 0, 0 for the exact 32-bit kernel), mode the MODE the kernel was instantiated with (0 score, 1 + ref_end,
 * 2 + both ends: a request the launcher serves with another instantiation, such as mode 1 of the 8..32-letter kernels or
 * mode 3 of the seeded passes' hand-backs, shows the one that ran; ZSW_LAUNCH_SEED_BAND alone can show 3, seed_band_kernel has
 * that instantiation: ends + "the maximum sits in one cell"). For the two seeded kinds (G, C) is the configuration of the length
 * class the pass ran for. Launches that decide on the device whether they do anything (ScoreArgsV2::gate_lo / gate_hi) are
 * recorded as issued; so is every tile of the tiled kernels. ZSW_LAUNCH_ROW_CHUNKS alone reads its fields otherwise: (kind, rows a
 * chunk owns, rows of overlap in front of them, number of chunks = grid rows) of the row-chunked score_kernel_v2 launch
 * (ScoreArgsV2::chunk_rows) whose ZSW_LAUNCH_V2 record comes next; a launch of whole rows has no such record. A launcher that finds no item on the host launches and records nothing. A strand-aware call reports the
 * launches of the last batch it staged. records: host memory for 4 * capacity uint32, may be NULL when capacity is 0; *out_n is
 * the number of launches. When capacity < *out_n nothing is written (ZSW_OK all the same): call again with that capacity. */
typedef enum zsw_launch_kind {
    ZSW_LAUNCH_V1_FAST = 0,        /* score_kernel, four-entry table (query residues >= 4 score 0) */
    ZSW_LAUNCH_V1_BIASED = 1,      /* score_kernel, biased byte table */
    ZSW_LAUNCH_V2 = 2,             /* score_kernel_v2 */
    ZSW_LAUNCH_WIDE = 3,           /* score_kernel_v2, LDS table (8..32 letters) */
    ZSW_LAUNCH_V1_FAST_REV = 4,    /* reverse pass of the ranges: score_kernel reversed, four-entry table */
    ZSW_LAUNCH_V1_BIASED_REV = 5,  /* ... biased byte table */
    ZSW_LAUNCH_WIDE_REV = 6,       /* ... LDS table */
    ZSW_LAUNCH_TILE_V2 = 7,        /* one tile of reads longer than the widest strip configuration */
    ZSW_LAUNCH_TILE_WIDE = 8,      /* ... LDS table */
    ZSW_LAUNCH_TILE_W32 = 9,       /* ... in 32-bit lanes (scores beyond the packed range; the reverse pass of such reads) */
    ZSW_LAUNCH_EXACT32 = 10,       /* exact32_kernel over a whole batch or length class */
    ZSW_LAUNCH_EXACT32_WORKLIST = 11, /* exact32_kernel over the device-side worklist (usually empty) */
    ZSW_LAUNCH_SEED_WINDOW = 12,   /* seeded pass: whole rows around the anchor (seed_window_kernel) */
    ZSW_LAUNCH_SEED_BAND = 13,     /* seeded pass: band of diagonals (seed_band_kernel), one record per tier */
    ZSW_LAUNCH_PRUNED = 14,        /* column-pruned pass (strip + window kernels of zsw_score_prune.hip), one record per pass */
    ZSW_LAUNCH_ROW_CHUNKS = 15     /* no kernel: the ZSW_LAUNCH_V2 record that follows is a row-chunked launch with these numbers */
} zsw_launch_kind;
zsw_error zsw_debug_score_launches(zsw_context* ctx, uint32_t* records, uint32_t capacity, uint32_t* out_n);

/* Reads of the context's last call that the seeded (or column-pruned) first pass handed back — no anchor, or a bound check
 * failed — and that were scored over all their cells (0 if the call did not take such a pass). Synchronises the device.
 * Read-as-profile role, every entry point (score, ends, ranges, alignment, 3-pass alignment): the hand-backs of the FORWARD pass.
 * The reversed seeded pass of the ranges and alignment calls is not counted: the reads it cannot settle are not rescored, they
 * go to the exact reverse kernel (or sw_simd_align's own second pass) with every read whose maximum is not in one cell.
 * Shared-profile role: zsw_score_shared_batch(_from) count the hand-backs of the role-swapped pass in the same way; the ends,
 * ranges and alignment calls of that role report 0, because their seeded passes rescore nothing — a read handed back joins the
 * reads with ties under the shared role's own kernel. After a strand-aware call: the hand-backs of the LAST score pass it ran —
 * the pass over the second batch (the reads scored on both strands), or the first pass if no read needed its other strand. After a panel call likewise: the hand-backs of the LAST score pass it ran —
 * the last member's list of the second round, or the last group of the first round if no read needed a second member.
 * Diagnostics for tests and bench.py. */
zsw_error zsw_prune_rescored(zsw_context* ctx, uint64_t* out_reads);

#ifdef __cplusplus
}
#endif
#endif /* ZOE_SW_H */
