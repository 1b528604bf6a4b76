/*
 * crbm_amd.h -- C-ABI of the MI355X-native CRBM training hot path.
 *
 * This is the drop-in boundary for the path that the reference
 * (schulter/crbm, secomo/convRBM.py) hands to Theano.  The reference has no
 * FFI layer: its inner boundary is the set of compiled-function handles made
 * in CRBM._compileTheanoFunctions (convRBM.py:453-515).  Every entry point
 * below replaces one of those handles (or the shared-variable accessors next
 * to them) one for one; the file:line it replaces is cited per function.
 *
 * Conventions
 *   - plain C, no C++/torch types; all array arguments are HOST pointers to
 *     C-contiguous float32 unless the name ends in _dev;
 *   - tensors use the reference's layouts: visible (n,1,A,L) with A = input_dims (4: DNA), hidden
 *     (n,K,1,Lh), filters (K,1,A,M), bias (1,K), c (1,A); the packed sums of a training step carry
 *     K*A*M weights per block and A letter counts (crbm_sums_count());
 *   - every function returns 0 on success, a negative crbm_status otherwise,
 *     and never throws; crbm_last_error() returns the message;
 *   - calls are synchronous w.r.t. the host unless the name ends in _async;
 *   - one handle owns one GPU (one process per GPU); a handle is not
 *     thread-safe; the library owns all device memory, the caller owns every
 *     host buffer it passes and may free it on return.
 *
 * Visible data must be exactly one-hot (reference sequences.py:28-31 builds
 * it that way); anything else returns CRBM_ERR_NOT_ONEHOT.
 */
#ifndef CRBM_AMD_H
#define CRBM_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CRBM_AMD_ABI_VERSION 5

typedef enum crbm_status {
  CRBM_OK = 0,
  CRBM_ERR_INVALID = -1,      /* bad argument / unsupported configuration */
  CRBM_ERR_HIP = -2,          /* a HIP runtime call failed                 */
  CRBM_ERR_NOT_ONEHOT = -3,   /* visible data is not exactly one-hot      */
  CRBM_ERR_NOT_BINARY = -4,   /* hidden state is not exactly 0/1          */
  CRBM_ERR_RCCL = -5,         /* an RCCL call failed / RCCL not loadable   */
  CRBM_ERR_NO_GPU = -6,       /* no usable HIP device                      */
  CRBM_ERR_IPC_TIMEOUT = -7   /* mapped-buffer all-reduce: a peer's sums never arrived (crbm_ipc_*) */
} crbm_status;

/* Hyper-parameters: the reference constructor's arguments
 * (convRBM.py:68-71) plus what Theano kept implicit. */
typedef struct crbm_config {
  int32_t num_motifs;          /* K                                   :111 */
  int32_t motif_length;        /* M  (1..64)                          :112 */
  int32_t input_dims;          /* A: 4 = DNA; 1..64 otherwise (generic kernels) :113 */
  int32_t doublestranded;      /* 0/1                                 :114 */
  int32_t batchsize;           /* number of persistent fantasy chains :115 */
  int32_t cd_k;                /* Gibbs steps per update              :121 */
  int32_t pooling;             /* hidden units compete in groups of this many
                                  positions (1..64; 1 = independent)  :120 */
  int32_t fantasy_hidden_len;  /* hidden length of the fantasy chains;
                                  the reference hard-codes 200        :168 */
  float learning_rate;         /*                                     :116 */
  float momentum;              /*                                     :117 */
  float rho;                   /* resolved target frequency (>0)  :136-140 */
  float lambda_rate;           /*                                     :119 */
  uint64_t seed;               /* Philox key (reference: wall clock   :155) */
  int32_t device;              /* HIP device ordinal                       */
  int32_t reserved;
} crbm_config;

typedef struct crbm_handle crbm_handle;

/* ---- lifetime ------------------------------------------------------------
 * crbm_create replaces CRBM.__init__'s shared-variable setup + the Theano
 * compile step (convRBM.py:127-175): allocates W,b,c, velocities (zero),
 * fantasy chains (zero) and compiles this model's kernels with hiprtc (cached
 * on disk).  W is zero until crbm_set_params. */
int crbm_create(const crbm_config* cfg, crbm_handle** out);
/* Runs only the kernel specialisation step of crbm_create (hiprtc compile of
 * the model's kernels into the on-disk cache); needs no GPU. */
int crbm_precompile(const crbm_config* cfg);
int crbm_destroy(crbm_handle* h);
/* Message of the last failed call on h (h may be NULL: last crbm_create). */
const char* crbm_last_error(const crbm_handle* h);
int crbm_abi_version(void);
/* Number of visible HIP devices (does not initialise a context). */
int crbm_device_count(void);

/* ---- shared-variable accessors (theano.shared get_value/set_value;
 * convRBM.py:133,149,152,158-173, used at :186-188,:233-235) --------------- */
int crbm_set_params(crbm_handle* h, const float* W, const float* b, const float* c);
int crbm_get_params(crbm_handle* h, float* W, float* b, float* c);
int crbm_set_velocities(crbm_handle* h, const float* vW, const float* vb, const float* vc);
int crbm_get_velocities(crbm_handle* h, float* vW, float* vb, float* vc);
/* fantasy_h / fantasy_h_prime, dense (batchsize,K,1,fantasy_hidden_len);
 * h_prime is ignored / may be NULL when single-stranded. */
int crbm_set_fantasy(crbm_handle* h, const float* hid, const float* hid_prime);
int crbm_get_fantasy(crbm_handle* h, float* hid, float* hid_prime);
/* Visible sample of the last Gibbs step, dense (batchsize,1,4,Lf+M-1). */
int crbm_get_fantasy_visible(crbm_handle* h, float* v);
/* Sampler state: key, Gibbs-step counter, evaluation counter, and the global
 * index of this rank's first chain / first data row (data-parallel runs). */
int crbm_set_rng(crbm_handle* h, uint64_t seed, uint32_t gibbs_step, uint32_t eval_step);
int crbm_get_rng(crbm_handle* h, uint64_t* seed, uint32_t* gibbs_step, uint32_t* eval_step);
int crbm_set_shard(crbm_handle* h, uint32_t chain_offset);

/* ---- training ------------------------------------------------------------
 * theano_trainingFct([D]) (convRBM.py:459-464, graph :373-438): one PCD-k
 * SGD+momentum update on mini-batch D (n,1,4,L); mutates W,b,c, velocities,
 * fantasy chains.  n may differ from batchsize (short last slice). */
int crbm_train_step(crbm_handle* h, const float* D, int32_t n, int32_t L);
/* Same, on rows [start,end) of a data set made resident with
 * crbm_dataset_upload (fit() uploads once, convRBM.py:612-615 then only
 * passes slice bounds). */
int crbm_dataset_upload(crbm_handle* h, const float* data, int32_t n, int32_t L);
/* Same from letter codes, one byte per base (0..3 = A,C,G,T: the map of
 * sequences.py:9-17; 0..input_dims-1 for any other alphabet), shape (n,L): 16x less host->device traffic than the
 * float one-hot array that sequences.py:101-117 builds. */
int crbm_dataset_upload_codes(crbm_handle* h, const uint8_t* codes, int32_t n, int32_t L);
/* A handle holds CRBM_DATASET_SLOTS resident data sets (fit() keeps the
 * training set in slot 0 and the test set of convRBM.py:617-625 in slot 1);
 * uploads and every *_resident call address the selected slot (default 0). */
#define CRBM_DATASET_SLOTS 2
int crbm_dataset_select(crbm_handle* h, int32_t slot);
int crbm_train_step_resident(crbm_handle* h, int32_t start, int32_t end);
/* The batch loop of fit() (convRBM.py:612-615) over the selected resident data
 * set: sequential slices of `batchsize` rows (convRBM.py:722-726), one PCD-k
 * update each, enqueued back to back with one host synchronisation at the end.
 * With a communicator, rank r takes rows [n*r/R, n*(r+1)/R) of every slice. */
int crbm_train_epoch_resident(crbm_handle* h, int32_t batchsize);
/* The same loop for a slot that holds only THIS rank's rows of every slice, in
 * slice order (rank r of R owns rows [n*r/R, n*(r+1)/R) of a slice of n rows):
 * every rank uploads 1/R of the `total_rows` data set instead of all of it.
 * `L` is the sequence length of the GLOBAL data set: a rank whose share is empty
 * has no resident rows to read it from, and every rank must normalise the
 * all-reduced sums with the same counts. */
int crbm_train_epoch_sharded(crbm_handle* h, int32_t batchsize, int32_t total_rows, int32_t L);
/* The persistent chain alone (convRBM.py:397-408): k Gibbs steps on all
 * fantasy chains, parameters frozen.  Benchmark entry. */
int crbm_gibbs_steps(crbm_handle* h, int32_t k);
int crbm_gibbs_steps_async(crbm_handle* h, int32_t k);
int crbm_sync(crbm_handle* h);
/* crbm_sync without the (blocking) read-back of the activity monitor: returns when everything launched has completed. */
int crbm_wait_idle(crbm_handle* h);
/* Times `launches` back-to-back launches of k Gibbs steps each with HIP
 * events on the library's stream; returns the total in milliseconds. */
int crbm_time_gibbs(crbm_handle* h, int32_t k, int32_t launches, float* total_ms);
/* Same for full training steps on resident rows [start,end). */
int crbm_time_train(crbm_handle* h, int32_t start, int32_t end, int32_t launches, float* total_ms);

/* ---- stand-alone passes (the graph builders the reference tests compile
 * directly, tests/testcrbm.py:165-171,:226-229) ---------------------------- */
/* _computeHgivenV(data, flip) (convRBM.py:269-275): any of act/prob/sample
 * may be NULL; each is (n,K,1,L-M+1).  Samples use Philox word 3 = rng_step. */
int crbm_h_given_v(crbm_handle* h, const float* v, int32_t n, int32_t L, int32_t flip,
                   uint32_t rng_step, float* act, float* prob, float* sample);
/* _computeVgivenH(h, hprime) (convRBM.py:317-325): hid (n,K,1,Lh) (any
 * finite values), hid_prime NULL or same shape; outputs (n,1,4,Lh+M-1),
 * each may be NULL. */
int crbm_v_given_h(crbm_handle* h, const float* hid, const float* hid_prime, int32_t n,
                   int32_t Lh, uint32_t rng_step, float* act, float* prob, float* sample);

/* ---- evaluation ------------------------------------------------------------
 * theano_getHitProbs (convRBM.py:507-514) -> (n,K,1,L-M+1). */
int crbm_hit_probs(crbm_handle* h, const float* v, int32_t n, int32_t L, float* out);
/* theano_freeEnergy (:501, graph :657-676) -> (n,) */
int crbm_free_energy(crbm_handle* h, const float* v, int32_t n, int32_t L, float* out);
/* theano_fePerMotif (:504, graph :678-697) -> (n,K) */
int crbm_free_energy_per_motif(crbm_handle* h, const float* v, int32_t n, int32_t L, float* out);
/* theano_evaluateData (:487-491) -> mean free energy, mean of a sampled H */
int crbm_eval_data(crbm_handle* h, const float* v, int32_t n, int32_t L, float* mfe, float* nmh);
/* theano_evaluateParams (:494-499) -> rms(W), IC, median IC */
int crbm_eval_params(crbm_handle* h, float* twn, float* ic, float* medic);

/* ---- data-set scale sweeps --------------------------------
 * The same evaluations fed with one byte per base (`_codes`, (n,L), 0..input_dims-1) or
 * with rows [start,end) of the selected resident data set (`_resident`), so
 * that the fp32 one-hot array of sequences.py:101-117 never has to exist.
 * Output pointers of the free-energy calls may be NULL (at least one is set). */
int crbm_hit_probs_codes(crbm_handle* h, const uint8_t* codes, int32_t n, int32_t L, float* out);
int crbm_hit_probs_resident(crbm_handle* h, int32_t start, int32_t end, float* out);
int crbm_free_energy_codes(crbm_handle* h, const uint8_t* codes, int32_t n, int32_t L, float* fe, float* fe_per_motif);
int crbm_free_energy_resident(crbm_handle* h, int32_t start, int32_t end, float* fe, float* fe_per_motif);
int crbm_eval_data_resident(crbm_handle* h, int32_t start, int32_t end, float* mfe, float* nmh);
/* The per-epoch evaluation loop of fit() (convRBM.py:616-625) over the selected resident data set in ONE call:
 * mini-batches of `batchsize` rows exactly as a loop over crbm_eval_data_resident would take them (same sampler
 * steps, one per batch), one host synchronisation.  Returns the mean over batches of the batches' mean free
 * energy and mean sampled hidden activity -- the two numbers of the reference's status line. */
int crbm_eval_epoch_resident(crbm_handle* h, int32_t batchsize, double* mean_fe, double* mean_nmh);
/* The three reductions of theano_getHitProbs' output that the reference's
 * analysis code uses, without materialising (n,K,1,Lh):
 *   hit_max  (n,K)  = P.max(axis=(2,3))    utils.py:154, :242-244
 *   hit_mean (n,K)  = P.mean(axis=(2,3))   utils.py:305
 *   position_mean (K,Lh) = P.mean(axis=(0,2))   utils.py:113-116
 * Any of the three pointers may be NULL. */
int crbm_hit_summary(crbm_handle* h, const float* v, int32_t n, int32_t L, float* hit_max, float* hit_mean,
                     float* position_mean);
int crbm_hit_summary_codes(crbm_handle* h, const uint8_t* codes, int32_t n, int32_t L, float* hit_max,
                           float* hit_mean, float* position_mean);
int crbm_hit_summary_resident(crbm_handle* h, int32_t start, int32_t end, float* hit_max, float* hit_mean,
                              float* position_mean);

/* ---- motif sites --------------------------------------------------------------
 * WHERE the motifs occur, without the dense (n,K,1,Lh) tensor of crbm_hit_probs.  The score of a hidden position is
 * the pooled probability of theano_getHitProbs (convRBM.py:507-514): single-stranded models have one per position,
 * sigma-pool(x + x'), strand 0; double-stranded models have two, the forward strand (+1, what crbm_hit_probs
 * reports) and the reverse-complemented filter (-1, _computeHgivenV(data, flip) of :269-275).
 * A site is a record with prob >= threshold (threshold in [0,1], else CRBM_ERR_INVALID); `start` is the hidden
 * position 0..L-M, the site covers letters [start, start+M); `seq` counts rows of the call (from `start` of the
 * resident form).  Records come sorted by (seq, motif, start, strand), + before -, the same bits in every run, for
 * every input form and every CRBM_SLAB_BYTES.  At most `capacity` of them are written to `sites`; `*count` is always
 * the exact total (threshold 0: n*K*S*(L-M+1), S = 2 double-stranded, else 1).  sites == NULL: no records, nothing
 * counted (count may then be NULL too).
 * Best site of every (seq, motif), (n,K) each: the largest prob over positions and strands, ties to the smaller start,
 * then to +.  best_start / best_strand / best_prob may each be NULL; all three NULL skips that work. */
typedef struct crbm_site {
  int32_t seq, motif, start, strand;   /* strand: +1, -1, or 0 (single-stranded model) */
  float prob;
} crbm_site;
int crbm_motif_sites(crbm_handle* h, const float* v, int32_t n, int32_t L, float threshold, int64_t capacity,
                     crbm_site* sites, int64_t* count, int32_t* best_start, int32_t* best_strand, float* best_prob);
int crbm_motif_sites_codes(crbm_handle* h, const uint8_t* codes, int32_t n, int32_t L, float threshold, int64_t capacity,
                           crbm_site* sites, int64_t* count, int32_t* best_start, int32_t* best_strand, float* best_prob);
int crbm_motif_sites_resident(crbm_handle* h, int32_t start, int32_t end, float threshold, int64_t capacity,
                              crbm_site* sites, int64_t* count, int32_t* best_start, int32_t* best_strand,
                              float* best_prob);

/* ---- stream scan: motif sites of whole records, any length, gaps allowed ---------
 * A stream is T codes, one byte each: 0..3 = A,C,G,T, 4 = no letter here (an N, an ambiguity code, the separator
 * between two records).  A window [s, s+M) is valid when all of its M codes are letters.  A valid window has the
 * scores crbm_motif_sites gives the same M letters anywhere in a row (the same bits), strands reported alike: 0
 * single-stranded, +1 / -1 double-stranded.  A site is a valid window, motif and strand with prob >= threshold; an
 * invalid window yields nothing; a stream shorter than M, or without a valid window, yields zero records and no error.
 * Records reuse crbm_site: seq is 0, start is the stream position of the window (hence T <= 2^31 - 1).  They come
 * sorted by (start, motif, strand), + before -: position order.  At most `capacity` of them are written to `sites`;
 * `*count` is always the exact total.  sites == NULL with capacity 0 only counts.  The same bits in every run and for
 * every CRBM_SLAB_BYTES (the stream goes through the device in segments of window starts, each with a halo of M - 1
 * letters, one byte per letter).
 * Served: DNA models without pooling on the specialised kernels, and those that run as slabs of motifs on them.
 * CRBM_ERR_INVALID: threshold outside [0,1], a code above 4, a negative T or capacity, T > 2^31 - 1; pooling > 1
 * (pool groups have no anchor in a stream), an alphabet other than DNA's, a model that runs on the generic kernels
 * alone (motifs beyond 64 letters).  The handle stays usable after a refusal. */
int crbm_scan_sites_codes(crbm_handle* h, const uint8_t* codes, int64_t T, float threshold, int64_t capacity,
                          crbm_site* sites, int64_t* count);

/* ---- score histogram: what the scan's scores look like on a background -----------
 * The stream scan with a histogram per (motif, strand) in place of records: which threshold gives which rate of sites,
 * and how surprising a site is.  Stream, windows and validity as crbm_scan_sites_codes.  The score of a valid window,
 * motif k and strand s is the log-odds x with prob = sigmoid(x), prob the probability the scan reports (x keeps
 * resolution where prob saturates); s = 0 is the + strand (the only one of a single-stranded model, S = 1), s = 1
 * the - strand of a double-stranded one (S = 2).
 * The bin rule: t = (x - lo) * inv_w with inv_w = nbins / (hi - lo) in fp32; the bin is 0 for t < 0, nbins - 1 for
 * t >= nbins, (int)t otherwise.  The first bin therefore holds everything below lo, the last everything at or above hi.
 * counts [K][S][nbins] is overwritten; *windows (may be NULL) is the number of valid windows.  For every (k, s),
 * sum_b counts[k][s][b] == *windows exactly.  Integer adds only: the same bits in every run, for every launch geometry
 * and every CRBM_SLAB_BYTES.  A stream shorter than M, or without a valid window, gives all zeros and no error.
 * Served: the models crbm_scan_sites_codes serves, when at least four motifs' counters (16 S nbins bytes) fit beside
 * the model's gather table in 160 KB of LDS.
 * CRBM_ERR_INVALID: what the scan refuses (pooling > 1, another alphabet, a generic-only model, a code above 4, T < 0,
 * T > 2^31 - 1); nbins < 1 or > 1024; lo or hi not finite, or lo >= hi; counts == NULL.  The handle stays usable
 * after a refusal; counts is then left as it was. */
int crbm_scan_histogram_codes(crbm_handle* h, const uint8_t* codes, int64_t T, float lo, float hi, int32_t nbins,
                              uint64_t* counts, int64_t* windows);

/* ---- record summaries: free energy and best site of every record of a stream --------
 * The per-sequence numbers of crbm_free_energy and crbm_motif_sites' best site for records of any length with gaps.
 * Stream, codes and window validity as crbm_scan_sites_codes.  rec_start holds nrec + 1 entries in the convention of
 * sequences.seqsToStream: record r is codes [rec_start[r], rec_start[r+1] - 1), one code 4 follows every record but the
 * last, rec_start[0] = 0 and rec_start[nrec] = T + 1.  A window belongs to the record its start lies in; the separator
 * keeps windows from spanning two records.  Per record r:
 *   windows[r]        = its valid windows                                                          (nrec) int64
 *   letters[r][a]     = its letters a = A,C,G,T                                                    (nrec,4) int64
 *   fe_per_motif[r,k] = - sum over its valid windows and the strands of softplus(x_k), x as crbm_variant_effects_codes
 *                       documents F (each strand of a double-stranded model, the forward activation alone of a
 *                       single-stranded one).  The hidden part only: the visible bias is NOT added to every column,
 *                       unlike crbm_free_energy_per_motif                                          (nrec,K) fp32
 *   fe[r]             = sum_k fe_per_motif[r,k] - sum_a letters[r][a] c[a]: the stream free energy F restricted to
 *                       the record; L * crbm_free_energy for a record of L letters without a gap   (nrec) fp32
 *   best_start, best_strand, best_prob [r,k]: the best site of (record, motif) with the scores of
 *                       crbm_scan_sites_codes (the same bits), start relative to the record, ties to the smaller start,
 *                       then to + (crbm_motif_sites' rule)                                          (nrec,K) int32, int32, fp32
 * A record without a valid window (shorter than M, empty, all N) has windows 0, a fe_per_motif row of exact zeros,
 * best_start -1, best_strand 0 and best_prob 0.
 * The free-energy sums are 64-bit fixed point: a window's softplus, summed over the strands in fp32 (+ before -), is
 * rounded to nearest into units of *unit once, and only integers are added from there; *unit = 2^-e is the finest
 * power of two, e <= 32, with 2^31 S (max(x_max, 0) + log 2) 2^e < 2^62, x_max = max_k (b_k + sum_j max_a W[k,a,j]):
 * it depends on the model alone and no stream a call accepts can overflow a sum.  A sum becomes fp32 with one rounding;
 * fe is formed in double (ascending k, then ascending letter) and rounded once.  Hence the same bits in every run, for
 * every launch geometry and every CRBM_SLAB_BYTES, and the rows of A ++ [4] ++ B are the rows of A followed by the
 * rows of B.  Any output may be NULL (at least one of those above is required when nrec > 0); unit may be NULL.
 * nrec == 0 requires T == 0 and writes nothing but *unit.
 * Served: exactly the models crbm_scan_sites_codes serves.
 * CRBM_ERR_INVALID: what the scan refuses (pooling > 1, another alphabet, a generic-only model, a code above 4, T < 0,
 * T > 2^31 - 1); a rec_start that does not start at 0, does not ascend, does not end with T + 1, or whose joints are
 * not codes 4 -- found on the host before anything is launched.  The handle stays usable after a refusal. */
int crbm_scan_records_codes(crbm_handle* h, const uint8_t* codes, int64_t T, const int64_t* rec_start, int64_t nrec,
                            int64_t* windows, int64_t* letters, float* fe, float* fe_per_motif, int32_t* best_start,
                            int32_t* best_strand, float* best_prob, double* unit);

/* ---- variant effects: what a substitution changes in the free energy of a stream ---
 * Given a stream and a list of variants (position, alternative letter): how much does each variant change the model's
 * free energy, and which motif gains or loses the site.  Stream, codes and window validity as crbm_scan_sites_codes:
 * codes 0..3 are letters, 4 is no letter, a window [s, s+M) is valid when all M codes are letters.  The free energy
 * of a stream is
 *   F(stream) = - sum_{valid windows s, strands, motifs k} softplus(x_{k,strand}(s)) - sum_{letters p} c[v_p],
 * the stream form of the F that crbm_mutagenesis documents: the hidden terms are those of crbm_free_energy (the
 * activation of each strand of a double-stranded model, the forward strand alone of a single-stranded one) -- not the
 * site score of the scan, which for single-stranded models adds both orientations.
 * For variant i = (pos_i, alt_i) with ref = codes[pos_i]:
 *   dfe_per_motif[i,k] = - sum over the valid windows s in [pos_i-M+1, pos_i] within [0, T-M] and the strands of
 *                          softplus(x_alt) - softplus(x_ref) for motif k: the hidden part only       (nvar,K) fp32
 *   dfe[i]             = sum_k dfe_per_motif[i,k] - (c[alt_i] - c[ref]), the motifs added in ascending k   (nvar) fp32
 *   windows[i]         = the number of valid windows that entered, 0..M                                  (nvar) int32
 * alt == ref gives exactly 0 everywhere.  ref == 4 (the variant sits on an N or a separator) gives windows = 0,
 * dfe = 0 and dfe_per_motif = 0.  A letter with no valid window around it (T < M, or gaps on both sides) gives
 * windows = 0 and dfe equal to the bias term alone.  A window that touches a gap elsewhere is left out, as the scan
 * leaves it out.  Every output of a variant depends on that variant and the stream alone: the same bits in every
 * run, for every CRBM_SLAB_BYTES (the list goes through the device in chunks, 2M - 1 context bytes per variant),
 * for every launch geometry and under any permutation or duplication of the list.  Variants may come in any order
 * and may repeat.  Any of the three outputs may be NULL; nvar == 0 succeeds and writes nothing.
 * Served: exactly the models crbm_scan_sites_codes serves.
 * CRBM_ERR_INVALID: pooling > 1, another alphabet, a generic-only model; all three outputs NULL; nvar < 0 or
 * > 2^31 - 1, a pos outside [0, T), an alt > 3, a code above 4, T < 0, T > 2^31 - 1 -- all found on the host before
 * anything is launched: the outputs are left as they were.  The handle stays usable after a refusal. */
int crbm_variant_effects_codes(crbm_handle* h, const uint8_t* codes, int64_t T, int64_t nvar, const int64_t* pos,
                               const uint8_t* alt, float* dfe, float* dfe_per_motif, int32_t* windows);

/* ---- allele effects: insertions, deletions and block substitutions -------------------
 * crbm_variant_effects_codes for alleles of any length.  Stream, codes and window validity as crbm_scan_sites_codes.
 * Variant i = (pos_i, R_i, alt_i[0..A_i)) replaces the R_i codes codes[pos_i .. pos_i+R_i) with the A_i letters
 * alt_codes[alt_off[i] .. alt_off[i+1]).  R = 0: a pure insertion in front of pos; A = 0: a pure deletion;
 * R = A = 1: the SNP.  Two haplotype contexts are built per variant, with left = codes [pos-M+1, pos) and
 * right = codes [pos+R, pos+R+M-1), positions outside the stream reading as code 4:
 *   refhap = left . codes[pos..pos+R) . right      R+M-1 window starts
 *   althap = left . alt . right                    A+M-1 window starts
 * A window is valid when all its M codes are letters.  With x as crbm_variant_effects_codes documents F (the
 * activations of crbm_free_energy per strand, not the scan's site score):
 *   S_hap,k            = sum over the valid windows of hap and the strands of softplus(x_k)
 *   dfe_per_motif[i,k] = -(S_alt,k - S_ref,k)                                                     (nvar,K) fp32
 *   dfe[i]             = sum_k dfe_per_motif[i,k] (ascending k) - (sum_j c[alt_j] - sum_j c[ref_j])   (nvar) fp32
 *   windows[i][0..1]   = the valid windows of refhap (0..R+M-1) and of althap (0..A+M-1)          (nvar,2) int32
 * dfe equals F(edited stream) - F(stream) over the whole stream: every other window is the same in both.
 * Exact zeros (dfe 0, the per_motif row 0, windows 0,0): R = A = 0, and a replaced span that holds a code 4 (the SNP
 * rule for a variant on an N).  A variant with no valid window on either haplotype gives a zero per_motif row and
 * the bias term alone.  Limits: R and A at most 65535 each; 0 <= pos and pos + R <= T (pos = T is allowed with
 * R = 0); alt codes 0..3; alt_off holds nvar+1 entries ascending from 0.
 * Every output of a variant depends on that variant's staged codes alone: the same bits in every run, for every
 * CRBM_SLAB_BYTES (the list goes through the device in chunks of R + A + 4M - 4 staged codes per variant), for every
 * launch geometry and under any permutation or duplication of the list.  Any of the three outputs may be NULL;
 * nvar == 0 succeeds and writes nothing.  Served: exactly the models crbm_scan_sites_codes serves.
 * CRBM_ERR_INVALID: what crbm_variant_effects_codes refuses, and a ref_len outside [0, 65535], an alt_off that does
 * not ascend from 0, an alt of more than 65535 letters, an alt code above 3, a span outside the stream -- all found on
 * the host before anything is launched: the outputs are left as they were.  The handle stays usable. */
int crbm_allele_effects_codes(crbm_handle* h, const uint8_t* codes, int64_t T, int64_t nvar,
                              const int64_t* pos, const int32_t* ref_len,
                              const int64_t* alt_off /* nvar+1, ascending from 0 */, const uint8_t* alt_codes,
                              float* dfe, float* dfe_per_motif, int32_t* windows);

/* ---- in-silico mutagenesis and pseudo-log-likelihood -----------------------------
 * WHICH bases matter.  With F(v) = L * crbm_free_energy(v), the unnormalised free energy of one sequence (derived from
 * theano_freeEnergyForData, convRBM.py:657-676: the hidden terms of all motifs and strands, pooled form when
 * pooling > 1, minus the visible bias term):
 *   dfe[n,p,a] = F(v_n with letter p replaced by a) - F(v_n)           (n,L,input_dims) fp32
 *   pll[n]     = sum_p -log sum_a exp(-dfe[n,p,a]) = sum_p log P(v_p | v_-p)      (n) fp32, <= 0
 * dfe[n,p,v_n[p]] is exactly 0; negative: the substitution fits the model better.  Only the motif_length windows
 * that cover p and the visible bias are evaluated (convRBM.py:657-676 restricted to what a substitution changes);
 * the mutated sequences never exist for specialised models without pooling (one fused kernel), every other model
 * expands a chunk of rows into its single-substitution copies on the device and runs its free-energy pass over them
 * (CRBM_MUT_FUSED=0 forces that path).  Either output may be NULL (pll alone never holds n*L*input_dims anywhere),
 * both NULL is CRBM_ERR_INVALID, and so is L < motif_length.  The same bits in every run, for every input form and
 * every CRBM_SLAB_BYTES. */
int crbm_mutagenesis(crbm_handle* h, const float* v, int32_t n, int32_t L, float* dfe, float* pll);
int crbm_mutagenesis_codes(crbm_handle* h, const uint8_t* codes, int32_t n, int32_t L, float* dfe, float* pll);
int crbm_mutagenesis_resident(crbm_handle* h, int32_t start, int32_t end, float* dfe, float* pll);

/* ---- annealed importance sampling: log Z and the normalised log-likelihood -------
 * (Neal 2001; Salakhutdinov & Murray 2008.)  Models on the specialised kernels, DNA alphabet, pooling == 1.  With
 * x, x' the bottom-up activations of the two strands (bias included, convRBM.py:238-243), S = 2 strands if
 * doublestranded else 1 and Lh = L - motif_length + 1:
 *   log p*_beta(v) = sum_{strands,k,s} softplus(beta x[k,s](v)) + sum_p (beta c[v_p] + (1 - beta) cA[v_p])
 * log p*_1(v) = -L * crbm_free_energy(v); cA = base_c (4) is the visible bias of the base-rate model (NULL: the
 * model's own c), whose partition function is log Z_A = L logsumexp(cA) + S K Lh ln 2.  The ladder betas[0..nbetas-1]
 * is non-decreasing inside [0,1].  Run r (global index run_offset + r) draws v_0 ~ softmax(cA) and does, for step t,
 *   logw += log p*_{betas[t+1]}(v_t) - log p*_{betas[t]}(v_t)
 *   h, h' ~ Bernoulli(sigmoid(betas[t+1] x(v_t))),  v_{t+1} ~ softmax(betas[t+1] (c + W^T h + rc(W)^T h') + (1 - betas[t+1]) cA)
 * with the counter layout and the 24-bit uniforms of the persistent chain under two kinds of their own (6: hidden,
 * 7: visible), keyed by `seed`: sequence word run_offset + r, step word 0 for v_0 and t + 1 for step t.  With
 * betas[0] = 0 and betas[nbetas-1] = 1, log Z ~= log Z_A + log mean_r exp(logw[r]) (the caller reduces, in double).
 *
 * crbm_ais does steps [t0,t1) of the ladder for `runs` runs.  t0 == 0: the runs start from the base-rate model and
 * logw from 0; t0 > 0: `state` (runs,L) letter codes and `logw` are read and continued.  On return logw (runs) holds
 * the accumulated log weights and state, if not NULL, v_{t1}.  The library cuts [t0,t1) into launches of at most
 * CRBM_AIS_STEPS steps (environment, default 64); logw[r] and state[r] have the same bits for every such cut, every
 * split of the runs over calls (run_offset) and every split of the ladder over calls.  The call reads the parameters
 * and changes nothing else of the handle: chains, last visible sample, sampler counters, velocities and resident data
 * sets are as before.  CRBM_ERR_INVALID: L < motif_length, runs <= 0, nbetas < 2, t0 / t1 outside
 * 0 <= t0 < t1 <= nbetas-1, a ladder that decreases, leaves [0,1] or is not finite, t0 > 0 without state, a run that
 * does not fit the LDS, pooling > 1, a model on the generic kernels, an alphabet other than DNA's. */
int crbm_ais(crbm_handle* h, int32_t L, int32_t runs, uint32_t run_offset, const float* betas, int32_t nbetas,
             int32_t t0, int32_t t1, const float* base_c, uint64_t seed, uint8_t* state, float* logw);

/* ---- data-parallel (new: the reference is single-device) -----------------
 * One process per GPU.  Rank 0 calls crbm_comm_unique_id and distributes the
 * 128 bytes by any host channel; every rank then calls crbm_comm_init.  After
 * that crbm_train_step* all-reduces (ncclSum, float32) one packed buffer of
 * raw statistic sums per step over RCCL/xGMI and every rank applies the same
 * update.  Layout of the packed buffer (floats), KAM = K*4*M:
 *   [vh_d KAM][vh_d' KAM][h_d K][h_d' K][sw KAM][sb K][v_d 4][n_d 1]
 *   [vh_m KAM][vh_m' KAM][h_m K][h_m' K][v_m 4][n_m 1]
 * (the primed blocks are present, zero-filled, also when single-stranded). */
#define CRBM_UNIQUE_ID_BYTES 128
int crbm_comm_unique_id(uint8_t id[CRBM_UNIQUE_ID_BYTES]);
int crbm_comm_init(crbm_handle* h, const uint8_t id[CRBM_UNIQUE_ID_BYTES], int32_t nranks, int32_t rank);
int crbm_comm_destroy(crbm_handle* h);
/* ncclBroadcast of W, b, c and the velocities from rank `root`: replicas must
 * start identical because only the statistic sums are reduced afterwards (the
 * reference's randn initialisation, convRBM.py:127-131, differs per process).
 * No-op without a communicator. */
int crbm_comm_broadcast_state(crbm_handle* h, int32_t root);
/* The same all-reduce WITHOUT a collective launch, for the ranks of one node (at most 8): every rank exports a
 * handle of its sums buffer (crbm_ipc_export, hipIpcGetMemHandle), the host ships the handles to all ranks by
 * any channel, every rank maps them (crbm_ipc_attach, `handles` = nranks x CRBM_IPC_HANDLE_BYTES in rank
 * order).  The column reduction of a training step then PUSHES the rank's packed sums into its slot of every
 * rank's buffer and raises its flag there; the update launch of every rank waits for the flags in its own
 * buffer and adds the slots in rank order (bit-identical on all ranks): no launch at all in place of
 * ncclAllReduce, and no read of remote memory on the critical path.  Alternative to crbm_comm_init, not to be
 * combined with it; replicas must start identical (crbm_amd.dist.attach ships rank 0's parameters first).
 * The wait is bounded in time (CRBM_IPC_TIMEOUT_MS, default 30 000, on the GPU's wall clock): once it has run out
 * no further update is applied (the parameters stay those of the last complete step) and every training entry
 * point and crbm_sync return CRBM_ERR_IPC_TIMEOUT; crbm_ipc_status reads the same word (*timed_out != 0).
 * While this form is attached the sums of a step go straight into the mapped buffers: what crbm_train_local-style
 * readers would find in the handle's own sums buffer is not current. */
#define CRBM_IPC_HANDLE_BYTES 64
int crbm_ipc_export(crbm_handle* h, uint8_t handle[CRBM_IPC_HANDLE_BYTES]);
int crbm_ipc_attach(crbm_handle* h, const uint8_t* handles, int32_t nranks, int32_t rank);
int crbm_ipc_detach(crbm_handle* h);
int crbm_ipc_status(crbm_handle* h, int32_t* timed_out);
int crbm_sums_count(const crbm_handle* h);
/* Split form of crbm_train_step for hosts that reduce the sums themselves:
 * local phase -> sums in `sums_out` (host, crbm_sums_count floats);
 * the caller reduces; apply consumes the reduced sums. */
int crbm_train_local(crbm_handle* h, const float* D, int32_t n, int32_t L, float* sums_out);
int crbm_train_apply(crbm_handle* h, const float* sums_in, int32_t L_data);
/* Times `launches` back-to-back all-reduces of the packed sums buffer alone
 * (HIP events on the library's stream; total in milliseconds): the collective's
 * share of a data-parallel training step.  The buffer's contents
 * are scratch at that point of a step; 0 ms without a communicator. */
int crbm_time_allreduce(crbm_handle* h, int32_t launches, float* total_ms);

/* ---- introspection used by bench/profiling ------------------------------- */
typedef struct crbm_launch_info {
  int32_t nq;            /* float4 quads of motifs the kernels are specialised for */
  int32_t group;         /* letters per gather-table group (G)                    */
  int32_t gibbs_grid, gibbs_block, gibbs_seqs_per_tile, gibbs_lds_bytes;
  int32_t stats_grid_x, stats_grid_y, stats_block, stats_lds_bytes;
  int32_t gibbs_sparse;  /* top-down variant of the Gibbs kernel: 1 = walk over set bits (default of every
                            model), 0 = dense tables (CRBM_TOPDOWN=dense, small models); fixed per handle  */
  int32_t activity_ppm;  /* hidden units on per million after the last crbm_sync / crbm_gibbs_steps, -1 = not read yet */
  int32_t stats_fused;   /* 1: the model half of the gradient statistics rides in the Gibbs launch of a training step */
  int32_t chain_parts;   /* plain chain launches (crbm_gibbs_steps*) go out as this many launches of a share of the chains
                            each, on streams of their own (the gibbs_* fields above then describe ONE of them)          */
  int32_t mutagenesis_route;  /* route of the last crbm_mutagenesis* call: 1 = fused kernel, 2 = general path, 0 = none yet */
} crbm_launch_info;
int crbm_get_launch_info(const crbm_handle* h, crbm_launch_info* out);
/* Device-copy bandwidth (float4 copy kernel, HIP events, read + written bytes
 * per second in GB/s) -- the measured ceiling bench.py reports beside the spec. */
int crbm_copy_bandwidth(crbm_handle* h, int64_t bytes, int32_t reps, float* gb_per_s);
/* Shader clock (MHz) during the launches of the last crbm_time_gibbs call, sampled by the chain kernel itself (one
 * block adds its duration in wall-clock ticks and in shader cycles): bench.py prices a step of overlapping launches in
 * shader cycles with it.  0 when unknown. */
int crbm_last_shader_clock(crbm_handle* h, float* mhz);
/* Chain kernel launches of this handle so far by the form of their geometry: compiled in (the kernels specialised on the
 * handle's launch shapes; CRBM_GEOM) and read from the arguments (every other launch).  Either may be null. */
int crbm_geometry_launches(const crbm_handle* h, int64_t* compiled_in, int64_t* run_time);
/* GPU resources this process holds through the library right now, over all handles and calls in flight:
 * counts[0..4] = device buffers, their bytes, streams, events, loaded code objects.  Every number returns to what it was
 * once the handles created since have been destroyed (a leak shows as a difference).  Needs no handle and no GPU. */
int crbm_live_resources(int64_t counts[5]);
/* Actual bytes of chain state one Gibbs launch reads+writes in HBM. */
int64_t crbm_gibbs_state_bytes(const crbm_handle* h);

/* ---- t-SNE of row features (utils.py:159-160, the TSNE().fit_transform of runTSNE) ------------------------------
 * Model-independent: the handle of any model lends its device, its stream and its error string.  Every pointer is
 * host memory; every call is complete when it returns.  Two components only.  No float atomics and sums in an order
 * fixed by n alone: the same inputs give the same bits in every run.  (Additive: the ABI version stays.)
 *
 * crbm_tsne_neighbors: for every row of X (n, D) float32 its k nearest OTHER rows by
 *   d2(i,j) = sum_d (x_id - x_jd)^2, float32, d ascending, difference form, no fused multiply-add,
 * ordered by (d2, j) ascending: idx (n, k) int32 and d2 (n, k) float32.  Exact (brute force): every row sees all n - 1
 * others.  CRBM_ERR_INVALID: n < 2 or n > 2^30, D < 1 or D > 256, k < 1, k > n - 1, k > 1024 (a wave keeps its list of
 * k (d2, j) pairs in the LDS), an X that is not finite.
 *
 * crbm_tsne_affinities: for every row the beta for which p_j = exp(-beta d2_j) / sum_j exp(-beta d2_j) over its k
 * distances has entropy log(perplexity) (natural logarithm), and that p (n, k); beta (n).  Bisection in float64 from
 * beta = 1, doubling or halving while a bound is open, 100 evaluations; the row's smallest d2 is subtracted inside the
 * exponent.  p is computed at the float32 beta that is returned.  A row that cannot reach the entropy -- all distances
 * equal, or at least `perplexity` of them tied for the smallest -- ends with a finite beta (2^100 at the most) and p
 * uniform over the tied.  CRBM_ERR_INVALID: n < 2, k outside [1, min(n - 1, 1024)], a perplexity that is not finite,
 * not positive or not below k + 1, a distance that is negative or not finite.
 *
 * crbm_tsne_descend: `iterations` steps of gradient descent on KL(P || Q), q_ij = w_ij / Z, w_ij = 1 / (1 + |y_i - y_j|^2),
 * Z = sum_i sum_{j != i} w_ij (exact, all n^2 pairs, float64 over the rows).  P is CSR (indptr (n + 1), indices, values),
 * kept on the device for the whole call; rows may be empty.  Gradient g_i = 4 (exaggeration A_i - R_i / Z) with
 * A_i = sum_{j in row i} P_ij w_ij (y_i - y_j) and R_i = sum_{j != i} w_ij^2 (y_i - y_j); update
 *   gains += 0.2 where velocity * g < 0, else gains *= 0.8, floored at 0.01;
 *   velocity = momentum * velocity - learning_rate * gains * g;  y += velocity.
 * y, velocity and gains are (n, 2) float32, read and written.  grad_last (n, 2), kl and z may be null; they receive the
 * gradient of the last iteration, and KL = sum P_ij log(max(P_ij, e) / max(w_ij / Z, e)), e = 2.2e-16, and Z at the y
 * that iteration started from.  iterations == 0 evaluates them at y and moves nothing.
 * CRBM_ERR_INVALID: n < 2 or n > 2^30, iterations < 0, an indptr that does not start at 0 or does not ascend (its last
 * entry is the number of values), an index outside [0, n).
 *
 * crbm_tsne_descend_ms: device time (HIP events) of the iterations of the handle's last crbm_tsne_descend call. */
int crbm_tsne_neighbors(crbm_handle* h, const float* X, int64_t n, int32_t D, int32_t k,
                        int32_t* idx, float* d2);
int crbm_tsne_affinities(crbm_handle* h, const float* d2, int64_t n, int32_t k, float perplexity,
                         float* p, float* beta);
int crbm_tsne_descend(crbm_handle* h, int64_t n, const int64_t* indptr, const int32_t* indices,
                      const float* values, float* y, float* velocity, float* gains, int32_t iterations,
                      float exaggeration, float learning_rate, float momentum,
                      float* grad_last, double* kl, double* z);
int crbm_tsne_descend_ms(crbm_handle* h, float* ms);

/* ---- Markov backgrounds: j-mer counts of a stream and exact sampling (the --bgfile of motif scanners) ------------
 * Model-independent: the handle of any model lends its device, its two streams and its error string.  Every pointer is
 * host memory; every call is complete when it returns.  Integer arithmetic only: the same inputs give the same bits in
 * every run, whatever the launch geometry, the segment size (CRBM_SLAB_BYTES) or the chunk length (CRBM_BG_CHUNK).
 * (Additive: the ABI version stays.)
 *
 * Codes are those of crbm_scan_sites_codes: 0..3 = A, C, G, T; 4 = no letter (a gap: N, a record separator).
 * A context is the last j <= order letters l_1 .. l_j, oldest first, with the index
 *   (4^j - 1) / 3 + sum_i l_i 4^(j - i);   0 is the empty context.
 * An order has (4^(order + 1) - 1) / 3 = 1, 5, 21, 85 contexts.
 *
 * crbm_stream_kmer_counts: for every j = 1 .. order + 1 and every j-mer, the number of positions p of the stream at
 * which all of codes[p .. p + j) are letters and spell it.  counts holds sum_j 4^j = 4, 20, 84, 340 entries: the 1-mers,
 * then the 2-mers, ..., each block indexed with the oldest letter most significant.  Long streams go to the device in
 * segments with a halo of `order` codes, on two buffer sets.
 * CRBM_ERR_INVALID: order outside [0, 3], T < 0 or T > 2^31 - 1, a null pointer (codes may be null when T == 0), a code
 * above 4.  counts is not written then, and the handle stays usable.
 *
 * crbm_background_sample: T codes of a Markov chain of the given order.  thr is the threshold table, (contexts, 3)
 * uint32, every row ascending: thr[ctx][i] = min(2^32 - 1, floor(2^32 sum_{a <= i} P(a | ctx))).  With P = pos0 + p:
 *   draw    u_p = word (P & 3) of philox4x32(c0 = (uint32)(P >> 2), c1 = (uint32)(P >> 34), c2 = 8 << 28, c3 = 0,
 *           key = (seed & 0xffffffff, seed >> 32)), seven rounds (8 is KIND_BACKGROUND of crbm_layout.h);
 *   gap     where tmpl holds a 4, out holds a 4 and the context becomes empty;
 *   letter  otherwise out[p] = a = #{ i < 3 : u_p >= thr[ctx][i] }, and the context becomes its last `order` letters
 *           with a appended (fewer while fewer have been drawn since the start or the last gap).
 * The context is empty at p = 0.  tmpl may be null: all letters.  A stream longer than one call takes is cut behind a
 * gap and every piece called with its pos0: the pieces are the stream of one call.  Exact: the chain is never
 * restarted from anything but its true context (composed transition maps, crbm_background.h).
 * CRBM_ERR_INVALID: order outside [0, 3], T < 0 or T > 2^31 - 1, pos0 < 0 or pos0 > 2^62, a null thr or out, a row of
 * thr that does not ascend, a code above 4 in tmpl.  out is not written then, and the handle stays usable.
 *
 * crbm_background_ms: device time (HIP events around the kernels of every segment, summed) of the handle's last
 * crbm_stream_kmer_counts or crbm_background_sample call. */
int crbm_stream_kmer_counts(crbm_handle* h, const uint8_t* codes, int64_t T, int32_t order, uint64_t* counts);
int crbm_background_sample(crbm_handle* h, const uint32_t* thr, int32_t order, int64_t T, int64_t pos0,
                           uint64_t seed, const uint8_t* tmpl, uint8_t* out);
int crbm_background_ms(crbm_handle* h, float* ms);

/* ---- The analytic null: the exact distribution of a quantised window score under a Markov background ---------------
 * Model-independent, like the Markov backgrounds above: the handle of any model lends its device, its main stream and
 * its error string.  Every pointer is host memory; the call is complete when it returns.  (Additive: the ABI version
 * stays.)
 *
 * crbm_score_distribution: R rows (a motif and strand each) of integer weights q (R, M, 4), q[r][j][a] >= 0 with
 * min_a q[r][j][.] = 0; the integer score of a window a_0 .. a_{M-1} is Q = sum_j q[r][j][a_j], within [0, G_r),
 * G_r = sum_j max_a q[r][j][.] + 1.  trans (contexts, 4) holds P(a | context) and init (contexts) the distribution of
 * the context in front of the window, contexts indexed as above, partial contexts included (they are ordinary states:
 * M < order + 1 is nothing special).  With next(s, a) the context behind s once a is appended:
 *   f_0[s][0] = init[s];   f_{j+1}[s'][Q] = sum_{(s, a): next(s, a) = s'} trans[s][a] * f_j[s][Q - q[r][j][a]];
 *   pmf[r][Q] = sum_s f_M[s][Q],   Q < G_r;   pmf[r][Q] = 0,   G_r <= Q < G.
 * All float64, products and adds rounded separately; the (at most five) terms of a cell are added with s ascending,
 * then a ascending, the contexts of the last sum in index order.  No atomics: the same inputs give the same bits
 * whatever the tile length (CRBM_NULL_TILE, default 1024 cells), the grouping of rows (the two state buffers of a group
 * of rows, 2 * contexts * max_r G_r * 8 bytes per row, stay within CRBM_NULL_BYTES, default 1 GiB) and the kernel
 * variant (CRBM_NULL_VARIANT: 0 plain gather, 1 sibling contexts through the LDS).
 * CRBM_ERR_INVALID, before anything is launched: a null pointer; R < 1; M outside [1, 512]; order outside [0, 3]; a
 * negative q or a position whose smallest q is not 0; G below the largest G_r or above 2^24; an entry of trans or init
 * that is negative or not finite; a row of trans that does not sum to 1 within 1e-9; a row whose state does not fit
 * CRBM_NULL_BYTES (the message says to use a larger step).  pmf is not written then, and the handle stays usable.
 *
 * crbm_null_ms: device time (HIP events around the kernels of every group of rows, summed) of the handle's last
 * crbm_score_distribution call. */
int crbm_score_distribution(crbm_handle* h, const int32_t* q, int32_t R, int32_t M, int32_t order, const double* trans,
                            const double* init, int64_t G, double* pmf);
int crbm_null_ms(crbm_handle* h, float* ms);

/* ---- Motif comparison: every placement of every query motif on every target motif, with exact p-values --------------
 * Model-independent, like the analytic null above: the handle of any model lends its device, its main stream and its
 * error string.  Every pointer is host memory; the call is complete when it returns.  (Additive: the ABI version stays.)
 *
 * A motif is w columns of four uint16 (A, C, G, T): x = clip(floor(p * 4096 + 0.5), 0, 4096).  qcols (qstart[K], 4) holds
 * the columns of the K queries, query k in the rows [qstart[k], qstart[k + 1]); tcols and tstart the N targets.  The
 * reverse complement of a motif has its columns reversed and its letters swapped A <-> T, C <-> G.  Two columns score
 *   D = sum_a (x_a - y_a)^2;   sim = 2^25 - min(D, 2^25);   bin = (sim * (bins - 1) + 2^24) >> 25   in [0, bins),
 * exact integers.  The pool is every target column (both != 0: and every column of every reverse complement), C columns.
 * For a query of width m:
 *   count[i][y]  the pool columns whose bin against query column i is y;   col[i][y] = (double)count[i][y] * invC
 *   pmf_{i,0} = [1];   pmf_{i,l}[x] = sum_{y = 0 .. bins - 1} pmf_{i,l-1}[x - y] * col[i+l-1][y],   x < G_l = l (bins - 1) + 1
 *   tail_{i,l}[G_l] = 0;   tail_{i,l}[x] = tail_{i,l}[x + 1] + pmf_{i,l}[x]
 * All float64, a product and an add rounded separately; the terms of a cell are added in ascending y from 0.0 (terms
 * outside the support are not added), the tails sequentially with x descending.  invC = 1.0 / C is the caller's.
 * Placement of a target of width n at offset o = -(n - 1) .. m - 1 (target column j under query column j + o):
 * i0 = max(0, o), j0 = max(0, -o), l = min(m - i0, n - j0); it is evaluated when l >= min(min_overlap, m, n), scores
 * S = sum_{t < l} bin(query column i0 + t, target column j0 + t) and has the p-value tail_{i0,l}[S].  Strand -1 places the
 * target's reverse complement by the same rule (both != 0 only).
 *
 * crbm_motif_compare: (K, N) outputs.  p_min: the smallest placement p-value of the pair; offset, strand (+1 / -1) and
 * overlap (l): that placement, ties on bit-equal p going to strand +1, then to the smaller offset; n_off: the
 * placements evaluated.  Everything is an integer up to the counts and one summation order from there: the same inputs
 * give the same bits whatever the launch geometry, the targets per block (CRBM_COMPARE_TILE, default 32, at most 64) and
 * the grouping of queries -- the tail tables of a group, sum_l (m - l + 1) (G_l + 1) * 8 bytes per query, and its 21
 * bytes per output pair stay within CRBM_COMPARE_BYTES (default 1 GiB).
 *
 * crbm_motif_compare_null: one query of width m.  counts (m, bins) uint32, and tail: the tables packed by start i
 * ascending, then l = 1 .. m - i ascending, G_l + 1 doubles each.
 *
 * CRBM_ERR_INVALID, before anything is launched: a null pointer; K or N < 1; a width outside [1, 64]; a start array
 * that does not begin at 0 or does not ascend; an entry above 4096; bins outside [2, 256]; min_overlap < 1; a pool
 * beyond 2^31 - 1 columns; invC outside (0, 1]; a single query whose tables and output row do not fit
 * CRBM_COMPARE_BYTES.  The outputs are not written then, and the handle stays usable.
 *
 * crbm_compare_ms: device time (HIP events around the kernels of every group, summed) of the handle's last
 * crbm_motif_compare or crbm_motif_compare_null call; stage_ms, where not null, receives three floats: counts, null,
 * placements. */
int crbm_motif_compare(crbm_handle* h, const uint16_t* qcols, const int32_t* qstart, int32_t K, const uint16_t* tcols,
                       const int32_t* tstart, int32_t N, int32_t bins, int32_t both, int32_t min_overlap, double invC,
                       double* p_min, int32_t* offset, int8_t* strand, int32_t* overlap, int32_t* n_off);
int crbm_motif_compare_null(crbm_handle* h, const uint16_t* qcols, int32_t m, const uint16_t* tcols, const int32_t* tstart,
                            int32_t N, int32_t bins, int32_t both, double invC, uint32_t* counts, double* tail);
int crbm_compare_ms(crbm_handle* h, float* ms, float* stage_ms);

#ifdef __cplusplus
}
#endif
#endif /* CRBM_AMD_H */
