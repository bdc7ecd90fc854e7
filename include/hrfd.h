/* include/hrfd.h -- C ABI of libhrfd.so, the MI355X (gfx950) implementation of the
 * HackRfDiags demodulation / modulation hot path.
 *
 * Plain C: opaque handles, raw pointers, sizes, int return codes.  No C++ or
 * torch types cross this boundary.  Every entry point names the reference
 * interface it stands in for (file:line under /root/reference/radioDiags).
 * The reference-named C++ classes in hackrfdiags_amd/csrc/shim/ are thin
 * wrappers over these calls (INTEGRATION.md shows how they are linked in).
 *
 * Conventions
 *   - return 0 on success, a negative HRFD_E* code on failure
 *     (hrfd_last_error() returns a human-readable message for the calling thread)
 *   - "channel" = one independent IQ stream = one IqDataProcessor + its four
 *     demodulators in the reference (Radio.cc:164-203)
 *   - one "block" = 262144 bytes of interleaved int8 IQ at 2.048 MS/s = 64 ms
 *     (hackRf/hackrf.c:101, DataConsumer.h:15) -> 512 int16 PCM samples at 8 kS/s
 *   - handles are single-caller for process calls; setters may be called from
 *     another thread and take effect at the next process call (the reference
 *     has the same unsynchronised CLI-thread setters)
 */
#ifndef HRFD_H
#define HRFD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HRFD_VERSION 1

/* error codes */
#define HRFD_OK            0
#define HRFD_EINVAL       -1   /* bad argument (NULL, a size the reference cannot take either: odd, 0, larger than its arrays) */
#define HRFD_ENODEV       -2   /* no HIP device / HIP runtime failure */
#define HRFD_ENOMEM       -3
#define HRFD_ESTATE       -4   /* handle misuse */

/* demodulator modes == IqDataProcessor::demodulatorType (hdr_diags/IqDataProcessor.h:21) */
#define HRFD_MODE_NONE 0
#define HRFD_MODE_AM   1
#define HRFD_MODE_FM   2
#define HRFD_MODE_WBFM 3
#define HRFD_MODE_LSB  4
#define HRFD_MODE_USB  5

#define HRFD_ALL_CHANNELS 0xffffffffu

#define HRFD_BLOCK_BYTES   262144u   /* DATA_CONSUMER_BUFFER_SIZE, hdr_diags/DataConsumer.h:15 */
#define HRFD_PCM_PER_BLOCK 512u      /* PCM_BLOCK_SIZE, hdr_diags/BasebandDataProcessor.h:16 */

typedef struct hrfd_rx hrfd_rx;       /* C channels of IqDataProcessor + demodulators */
typedef struct hrfd_demod hrfd_demod; /* C channels of one {Am,Fm,WbFm,Ssb}Demodulator */
typedef struct hrfd_mod hrfd_mod;     /* C channels of SsbModulator / interpolateSignal */

const char *hrfd_last_error(void);
int hrfd_version(void);
/* number of visible HIP devices (0 when there is no GPU; never fails) */
int hrfd_device_count(void);

/* ------------------------------------------------------------------------------
 * Receive, outer boundary.
 * Replaces: IqDataProcessor::IqDataProcessor / ~IqDataProcessor
 *           (src_diags/IqDataProcessor.cc:56-160) for n_channels streams at once,
 *           together with the four demodulator objects Radio.cc:179-197 creates.
 * device < 0 selects the current HIP device.
 */
int hrfd_rx_create(uint32_t n_channels, int device, hrfd_rx **out);
int hrfd_rx_destroy(hrfd_rx *h);

/* IqDataProcessor::setDemodulatorMode (IqDataProcessor.cc:346-375); LSB/USB also
 * select the SSB demodulator's sideband, as the reference does. */
int hrfd_rx_set_mode(hrfd_rx *h, uint32_t channel, int mode);
/* {Am,Fm,WbFm,Ssb}Demodulator::setDemodulatorGain (e.g. WbFmDemodulator.cc:299) */
int hrfd_rx_set_gain(hrfd_rx *h, uint32_t channel, int mode, float gain);
/* IqDataProcessor::setSignalDetectThreshold (IqDataProcessor.cc:392-405), dBFS */
int hrfd_rx_set_threshold(hrfd_rx *h, uint32_t channel, int32_t threshold);
/* X::resetDemodulator (e.g. WbFmDemodulator.cc:265-278; NB: the WBFM de-emphasis
 * filter is not reset there, and is not reset here) */
int hrfd_rx_reset_demod(hrfd_rx *h, uint32_t channel, int mode);

/* IqDataProcessor::acceptIqData (IqDataProcessor.cc:926-1038) for every channel,
 * n_blocks consecutive blocks per channel in one call.  Host buffers:
 *   iq            [n_channels][n_blocks][block_bytes] int8, interleaved I,Q, 2.048 MS/s
 *   block_bytes   ANY even count, 2 .. 262144, like the reference: DataConsumer::acceptData clips longer buffers and
 *                 counts and PASSES ON shorter ones (DataConsumer.cc:229-241, :341-343; a USB transfer that ends early,
 *                 hackRf/hackrf.c:1443), and every decimator keeps its commutator position between calls
 *                 (Decimator_int16.cc:321-362).  What comes out per call is the reference's: the front end holds back
 *                 p = 0..7 IQ samples (hrfd_rx_pending_samples), a call completes floor((p + block_bytes/2) / 8) samples
 *                 at 256 kS/s, the Fs/4 rotation restarts at every call, the squelch mean is the call's own, the
 *                 demodulator emits what its three stages complete.  Odd counts are refused: the reference's Q loop then
 *                 reads bufferPtr[byteCount] (IqDataProcessor.cc:474) -- pass byteCount + 1 to get its result.  A call
 *                 too short to complete one 256 kS/s sample makes the reference divide by zero (SignalDetector.cc:255);
 *                 here it reports magnitude 0.
 *                 Speed: multiples of 1024 on a handle whose blocks all were multiples of 512 run on the streaming
 *                 kernels; other multiples of 512 (a transfer some USB packets short: 261632) pass through the exact
 *                 general kernel and the stream is back on the streaming kernels with the next full block; the first
 *                 block of any OTHER length moves the handle to the general kernel for good.
 *   gain_db       radio_adjustableReceiveGainInDb (Radio.cc:15) at call time
 *   pcm           [n_channels][n_blocks][hrfd_rx_pcm_capacity(block_bytes)] int16: a row holds n_pcm samples (out)
 *   n_pcm         [n_channels][n_blocks] samples actually produced (block_bytes/512 for whole multiples of 512 on an
 *                 open gate); 0 when squelched / mode NONE (the reference then makes no PCM callback)   (out)
 *   magnitude     [n_channels][n_blocks] Squelch::getSignalMagnitude() (out, may be NULL = not wanted.  A device-entry
 *                 batch of WBFM channels given NULL does not compute it at all while no squelch gate of the bank can
 *                 close -- every threshold <= -42 - gain_db, the reference's default of -200 among them: PCM, n_pcm,
 *                 signal_allowed and the carried state do not depend on it then, and the launch is faster for it)
 *   signal_allowed[n_channels][n_blocks] Squelch::run() result       (out, may be NULL)
 *   iq256k_opt    [n_channels][n_blocks][hrfd_rx_iq256_capacity(block_bytes)] decimatedData after the Fs/4 mix -- what
 *                 `enable iqdump` sends by UDP; block_bytes/8 bytes for multiples of 16   (out, may be NULL)
 * Blocking: returns when the outputs are in the host buffers.
 */
int hrfd_rx_process_block(hrfd_rx *h, const int8_t *iq, uint32_t block_bytes,
                          uint32_t n_blocks, uint32_t gain_db, int16_t *pcm,
                          uint32_t *n_pcm, uint32_t *magnitude,
                          uint8_t *signal_allowed, int8_t *iq256k_opt);
/* Row lengths of the outputs above: ceil(block_bytes / 512) PCM samples, 2 * ceil(block_bytes / 16) bytes of the
 * 256 kS/s stream (what a call can complete at most, whatever the decimators hold). */
uint32_t hrfd_rx_pcm_capacity(uint32_t block_bytes);
uint32_t hrfd_rx_iq256_capacity(uint32_t block_bytes);
/* IQ samples the front end's three half-band decimators hold back after the calls so far (0..7, the same for every
 * channel of the handle; 0 while every block was a multiple of 16 bytes): the NEXT call of block_bytes bytes completes
 * floor((pending + block_bytes / 2) / 8) samples at 256 kS/s = IqDataProcessor::reduceSampleRate's return value / 2
 * (IqDataProcessor.cc:429-500).  Waits for the handle's last call. */
int hrfd_rx_pending_samples(hrfd_rx *h, uint32_t *pending);

/* IqDataProcessor::reduceSampleRate (IqDataProcessor.cc:429-500; public in the reference, not called by the
 * application): one block of every channel through the three half-band stages only -- the decimator pipelines advance,
 * the squelch and the demodulators are left alone.  iq [n_channels][block_bytes]; iq256k [n_channels][block_bytes/8]
 * receives the stream WITH the Fs/4 rotation (the front end is fused with the mixer here; the rotation is exactly
 * invertible, the shim class takes it out again).  Blocking; not to be called while another thread changes the
 * handle's modes (it parks them for the duration of the call). */
int hrfd_rx_reduce_sample_rate(hrfd_rx *h, const int8_t *iq, uint32_t block_bytes, int8_t *iq256k);

/* Same work with every buffer already resident in device memory (HBM); this is
 * the entry the batched benchmark drives.  d_iq is [n_channels][n_blocks]
 * [block_bytes] with channel_stride bytes between channels; block_bytes and the rows of the outputs as above
 * (d_n_pcm may be NULL; a d_iq256k_opt row is written up to the call's own count).  Asynchronous on
 * `stream` (a hipStream_t, NULL = the handle's own stream).  Optional outputs
 * may be NULL.  When n_blocks > 1 the call is one continuous stream per channel (or, for small banks and odd block
 * sizes, blocks demodulated concurrently): it speculates that every squelch gate in the batch is open and that the
 * WBFM de-emphasis tiles re-synchronise; both assumptions are verified on the device.  A gate that closes
 * inside the batch is repaired on the device as well: a gated pass behind the batch launch redoes the channels
 * concerned exactly (the stream of the blocks the squelch tracker allows).  hrfd_rx_sync() reports what is left.
 * Stream ordering is the caller's: the handle's own stream is non-blocking, so buffers that
 * were filled or cleared on another stream (e.g. a framework's default stream) must be
 * complete -- or `stream` must be that stream -- before this call.
 */
int hrfd_rx_process_device(hrfd_rx *h, const int8_t *d_iq, uint64_t channel_stride,
                           uint32_t block_bytes, uint32_t n_blocks, uint32_t gain_db,
                           int16_t *d_pcm, uint32_t *d_n_pcm, uint32_t *d_magnitude,
                           uint8_t *d_signal_allowed, int8_t *d_iq256k_opt,
                           void *stream);
/* Waits for the last hrfd_rx_process_device call.  *n_violations (may be NULL)
 * receives the number of CHANNELS that did not commit in that call (0 = every output is exact and every state
 * advanced).  The verdict is per channel: a channel that verified clean has advanced its state and
 * its outputs are exact; a failed channel has NOT advanced and the caller should
 * resubmit that channel one block per call (n_blocks == 1 is always exact) --
 * hrfd_rx_failed_channels says which, hrfd_rx_process_block does all of this by
 * itself.  Closed squelch gates are not failures (the device repairs them, see above) unless the batch has more
 * than 64 blocks or runs on the block kernels (small banks, odd block sizes).  (hrfd_rx_process_block runs a call of
 * more than 64 blocks as chunks of at most 64, each with the device's repair behind it: a caller of this entry that wants
 * the same keeps its calls at 64 blocks or fewer.) */
int hrfd_rx_sync(hrfd_rx *h, uint32_t *n_violations);
/* out[c] != 0 for the channels of that call that did not commit (n = n_channels). */
int hrfd_rx_failed_channels(hrfd_rx *h, uint8_t *out, uint32_t n);

/* ------------------------------------------------------------------------------
 * Receive, inner boundary: one demodulator class, n_channels instances.
 * Replaces: X::X(pcmCallbackPtr), X::acceptIqData(int8_t*,uint32_t),
 *           X::setDemodulatorGain, X::resetDemodulator,
 *           SsbDemodulator::set{Lsb,Usb}DemodulationMode
 *           (WbFmDemodulator.h:23-31, FmDemodulator.h:23-31, AmDemodulator.h:23-31,
 *            SsbDemodulator.h:24-34).
 * Input is 256 kS/s int8 IQ, already mixed; bytes_per_channel any even count <= 32768 (the reference's fixed member
 * arrays; its loops take any count and the decimators keep their positions, e.g. WbFmDemodulator.cc:395, :460-500).
 * pcm [n_channels][hrfd_demod_pcm_capacity(bytes_per_channel)], n_pcm [n_channels] (may be NULL) the samples produced:
 * bytes_per_channel / 64 for whole multiples of 64.  The PCM callback of the reference becomes the pcm/n_pcm output
 * pair; the C++ shim invokes the callback.
 */
int hrfd_demod_create(int mode, uint32_t n_channels, int device, hrfd_demod **out);
int hrfd_demod_destroy(hrfd_demod *h);
int hrfd_demod_reset(hrfd_demod *h, uint32_t channel);
int hrfd_demod_set_gain(hrfd_demod *h, uint32_t channel, float gain);
int hrfd_demod_set_sideband(hrfd_demod *h, uint32_t channel, int lsb);
int hrfd_demod_process(hrfd_demod *h, const int8_t *iq256k, uint32_t bytes_per_channel,
                       int16_t *pcm, uint32_t *n_pcm);
uint32_t hrfd_demod_pcm_capacity(uint32_t bytes_per_channel);   /* ceil(bytes_per_channel / 64) */

/* ------------------------------------------------------------------------------
 * Block transport in front of hrfd_rx.  Replaces the role of
 * DataConsumer (src_diags/DataConsumer.cc:219-262 acceptData: copy into a ring of messages and
 * queue; :319-351 the consumer thread calling IqDataProcessor::acceptIqData) for many channels:
 * a ring of n_slots pinned host batches [n_channels][n_blocks][block_bytes]; a submitted batch
 * is copied to the device, demodulated and its results copied back on separate streams, so the
 * transfer of one batch runs under the kernels of the previous one.  Results are the sequential
 * ones (a batch whose speculation fails is replayed exactly, with the batches in flight behind it).
 *   producer:  hrfd_ingest_acquire (pinned input buffer of the next free slot; HRFD_ESTATE when
 *              none is free) -> fill -> hrfd_ingest_submit (returns at once)
 *   consumer:  hrfd_ingest_collect (oldest submitted batch; blocks; pcm [C][B][hrfd_rx_pcm_capacity(block_bytes)],
 *              n_pcm / magnitude / signal_allowed [C][B]; pointers valid until that slot is
 *              acquired again; any of the four out pointers may be NULL)
 * The rx handle must not be used by other calls while batches are in flight.
 * hrfd_ingest_destroy with batches still in flight collects them first: afterwards the rx handle is in the state a
 * sequential caller reaches after every SUBMITTED batch -- channels that failed in an uncollected batch are replayed
 * (their results are discarded), no channel is left marked as failed, and the stream may go on with any hrfd_rx_* call.
 * A slot that was acquired and never submitted is not a batch.  Destroy the transport before its rx handle.
 */
typedef struct hrfd_ingest hrfd_ingest;
int hrfd_ingest_create(hrfd_rx *rx, uint32_t block_bytes, uint32_t n_blocks, uint32_t n_slots,
                       hrfd_ingest **out);
int hrfd_ingest_destroy(hrfd_ingest *g);
int hrfd_ingest_acquire(hrfd_ingest *g, int8_t **iq_slot);
int hrfd_ingest_submit(hrfd_ingest *g, uint32_t gain_db);
int hrfd_ingest_collect(hrfd_ingest *g, const int16_t **pcm, const uint32_t **n_pcm,
                        const uint32_t **magnitude, const uint8_t **signal_allowed);
int hrfd_ingest_replayed(hrfd_ingest *g, uint64_t *n_batches);

/* ------------------------------------------------------------------------------
 * One host process, several devices.  The reference wires its whole receive path into one process
 * (src_diags/Radio.cc:164-237: one IqDataProcessor, its demodulators, one DataConsumer thread); a host that drives many
 * channels on the GPUs of a node stays one process too.  Channels share nothing, so n_devices devices are n_devices
 * contiguous channel shards -- shard g owns channels [first, first + count) of hrfd_fanout_channel_range: sizes differ
 * by at most one -- each an hrfd_rx of its own on its device, state pinned there.  No collective: IQ that lands on one
 * device leaves it as one peer copy per shard, every copy on the receiving shard's stream (xGMI is point to point: the
 * links out of the source work at the same time; in-process, no RCCL bootstrap), and the PCM comes back the same way.
 * devices[] may name a device more than once (several shards on one GPU).
 *   hrfd_fanout_scatter   d_iq_all [n_channels][n_blocks][block_bytes] on src_device -> the shards' input buffers;
 *                         src_stream: the stream that produced d_iq_all (awaited on the devices), NULL = complete
 *   hrfd_fanout_input     instead of scatter: the shard's own input buffer, for a host that feeds every device itself
 *   hrfd_fanout_process   IqDataProcessor::acceptIqData (IqDataProcessor.cc:926-1038) for every channel, n_blocks
 *                         blocks each, all devices at once, asynchronous
 *   hrfd_fanout_collect   waits, replays exactly what failed its speculation (as hrfd_rx_process_block does), gathers
 *                         pcm [n_channels][n_blocks][hrfd_rx_pcm_capacity(block_bytes)] and n_pcm [n_channels][n_blocks] (may be NULL)
 *                         into buffers on dst_device; *n_replayed (may be NULL) = channels replayed
 * One batch at a time: from a successful hrfd_fanout_process until its hrfd_fanout_collect the batch is IN FLIGHT, and
 * hrfd_fanout_scatter, hrfd_fanout_input and hrfd_fanout_process answer HRFD_ESTATE and leave it untouched (collect
 * replays failed channels from the shards' input buffers with the batch's block size and gain_db; a second scatter or
 * process would replace them).  hrfd_fanout_collect without a batch in flight and hrfd_fanout_process before any
 * scatter / input are HRFD_ESTATE too; a NULL handle or destination is HRFD_EINVAL.
 * The setters take channel numbers of the whole bank (HRFD_ALL_CHANNELS: every shard).
 * (The multi-process counterpart -- one rank per GPU, RCCL -- is hackrfdiags_amd/shard.py, used by bench.py --gpus N.)
 */
typedef struct hrfd_fanout hrfd_fanout;
int hrfd_fanout_channel_range(uint32_t n_channels, uint32_t n_shards, uint32_t shard, uint32_t *first, uint32_t *count);
int hrfd_fanout_create(uint32_t n_channels, const int *devices, uint32_t n_devices, hrfd_fanout **out);
int hrfd_fanout_destroy(hrfd_fanout *f);
int hrfd_fanout_shards(hrfd_fanout *f, uint32_t *n_shards);
int hrfd_fanout_set_mode(hrfd_fanout *f, uint32_t channel, int mode);
int hrfd_fanout_set_gain(hrfd_fanout *f, uint32_t channel, int mode, float gain);
int hrfd_fanout_set_threshold(hrfd_fanout *f, uint32_t channel, int32_t threshold);
int hrfd_fanout_scatter(hrfd_fanout *f, int src_device, const int8_t *d_iq_all, uint32_t block_bytes, uint32_t n_blocks,
                        void *src_stream);
int hrfd_fanout_input(hrfd_fanout *f, uint32_t shard, uint32_t block_bytes, uint32_t n_blocks, int8_t **d_iq,
                      uint32_t *first_channel, uint32_t *n_shard_channels);
int hrfd_fanout_process(hrfd_fanout *f, uint32_t gain_db);
int hrfd_fanout_collect(hrfd_fanout *f, int dst_device, int16_t *d_pcm_all, uint32_t *d_n_pcm_all, uint32_t *n_replayed);

/* ------------------------------------------------------------------------------
 * Transmit: PCM -> int8 IQ through the 8-stage x256 half-band interpolator.
 * kind HRFD_MOD_SSB replaces SsbModulator::acceptData (SsbModulator.cc:455-470)
 * incl. set{Lsb,Usb}ModulationMode / resetModulator (SsbModulator.h:23-35);
 * kind HRFD_MOD_INTERP replaces the signals/interpolateSignal tool
 * (signals/interpolateSignal.cc:250-374: int16 IQ pairs in, its own stage-1 table).
 */
#define HRFD_MOD_SSB    1
#define HRFD_MOD_INTERP 2
/* kinds HRFD_MOD_AM / HRFD_MOD_FM replace AmModulator::acceptData (AmModulator.cc:381-395,
 * modulateSignal :574-612) and FmModulator::acceptData (FmModulator.cc:393-407, modulateSignal
 * :586-627: an 8 kS/s Nco driven by deviation * pcm / 32768), same x256 cascade and tables;
 * PCM in, as for SSB.  FM goes through cosf / sinf: bit-exact on a glibc host since round 5 (hrfd_libm_variant() below). */
#define HRFD_MOD_AM     3
#define HRFD_MOD_FM     4
/* kind HRFD_MOD_WBFM replaces WbFmModulator::acceptData (WbFmModulator.cc:341-356: PCM x32,
 * a 256 kS/s Nco with runFast's table driven by deviation * x / 1024, x900, then x8): bit-exact
 * (the tables are built with the host's libm like the reference's). */
#define HRFD_MOD_WBFM   5
/* kinds HRFD_MOD_SIG_* replace the baseband generators of signals/ piped into interpolateSignal
 * (signals/makeThem.sh, generateBaseband.sh: `./a.out < pcm.raw | ./interpolateSignal > x.iq`):
 * am.cc:40-52 ((pcm*0.8 + 65536)/4 on both rails), dsb.cc:38-46 (pcm/4), pm.cc:41-53
 * (phase = pcm/60000*pi, 16000*cos/sin), fm.cc:44-77 (theta += pcm/65536*3.5, wrapped at +-2pi).
 * PCM in, int8 IQ at 2.048 MS/s out -- the .iq files that `load iqfile` plays (hrfd_play).
 * All four bit-exact (PM and FM go through cosf / sinf: on a glibc host, hrfd_libm_variant() below). */
#define HRFD_MOD_SIG_AM  6
#define HRFD_MOD_SIG_DSB 7
#define HRFD_MOD_SIG_PM  8
#define HRFD_MOD_SIG_FM  9
/* Which build of glibc's sinf / cosf the HOST's libm is: the reference reaches them through cos(float) / sin(float)
 * (Nco.cc:186-199, FmModulator.cc:600, signals/pm.cc, fm.cc) and the device restates that build bit for bit.
 * 1 = FMA build, 0 = without FMA, -1 = neither probed build (a libm that is not glibc's: the device follows the FMA
 * build and the FM modulator, Nco::run and the pm / fm generators may then differ from that host's libm by +-1 LSB). */
int hrfd_libm_variant(void);
int hrfd_mod_create(int kind, uint32_t n_channels, int device, hrfd_mod **out);
int hrfd_mod_destroy(hrfd_mod *h);
int hrfd_mod_reset(hrfd_mod *h, uint32_t channel);
int hrfd_mod_set_sideband(hrfd_mod *h, uint32_t channel, int lsb);
/* AmModulator::setModulationIndex (AmModulator.cc:329-336; default 0.8, accepted in [0, 1]) */
int hrfd_mod_set_modulation_index(hrfd_mod *h, uint32_t channel, float index);
/* FmModulator::setFrequencyDeviation (FmModulator.cc:336-346; default 3500 Hz) and
 * WbFmModulator::setFrequencyDeviation (WbFmModulator.cc:307-318; default 70000 Hz) */
int hrfd_mod_set_deviation(hrfd_mod *h, uint32_t channel, float deviation_hz);
/* pcm [n_channels][n_per_channel] int16 (SSB) or [n_channels][2*n_per_channel]
 * int16 IQ pairs (INTERP); iq_out [n_channels][512*n_per_channel] int8;
 * *out_bytes = 512*n_per_channel (bytes per channel, as the reference returns).
 * hrfd_mod_process_device takes device buffers and is asynchronous on `stream` (a hipStream_t, NULL = the handle's own);
 * hrfd_mod_sync waits for the handle's last launch.  Setters never wait for the device: what a setter changed goes to
 * the device with the next call, ahead of its launch.  Calls may use different streams: each launch is ordered on the
 * device behind the handle's previous one (the pipelines and phase accumulators are the handle's).  A call whose size
 * does not fit the launches' 32-bit arithmetic -- 8 ceil(n_channels / 8) * ceil(n_per_channel / 128) above 2^24 - 1, or
 * for HRFD_MOD_WBFM n_per_channel above 67108735 -- is refused with HRFD_EINVAL before any device is touched. */
int hrfd_mod_process(hrfd_mod *h, const int16_t *pcm, uint32_t n_per_channel,
                     int8_t *iq_out, uint32_t *out_bytes);
int hrfd_mod_process_device(hrfd_mod *h, const int16_t *d_pcm, uint32_t n_per_channel,
                            int8_t *d_iq_out, void *stream);
int hrfd_mod_sync(hrfd_mod *h);

/* ------------------------------------------------------------------------------
 * The transmit side's PCM ring, one per channel (host code).  Same slots, table
 * and pacing policy as BasebandDataProcessor (src_diags/BasebandDataProcessor.cc: ctor :41-84,
 * getNextUnfilledBuffer :410-425, getNextFilledBuffer :476-606 -- more than 10 blocks of lag
 * drops one, fewer than 6 sends the previous one again, not running reads zeros --, start/stop
 * :306-356).  hrfd_txring_read_batch gathers one 512-sample block per channel into
 * batch[n_channels][512], the input of hrfd_mod_process(h, batch, 512, ...).
 * stats: {produced, consumed, dropped, added, writer index, reader index}.
 */
typedef struct hrfd_txring hrfd_txring;
int hrfd_txring_create(uint32_t n_channels, hrfd_txring **out);
int hrfd_txring_destroy(hrfd_txring *r);
int hrfd_txring_set_running(hrfd_txring *r, uint32_t channel, int running);
int hrfd_txring_write(hrfd_txring *r, uint32_t channel, const int16_t *pcm512);
int hrfd_txring_read_batch(hrfd_txring *r, int16_t *batch);
int hrfd_txring_stats(hrfd_txring *r, uint32_t channel, uint32_t *out6);

/* ------------------------------------------------------------------------------
 * Cyclic playback of an .iq file (raw int8 IQ at 2.048 MS/s): DataProvider::loadIqFile /
 * getIqData (src_diags/DataProvider.cc:235-300, 122-131, 174-231) with the file image resident in
 * HBM and one read position per channel, so that one recording drives many receive channels
 * (SURVEY 8f rank 4).  hrfd_play_get_device fills d_out[c][bytes_per_channel] (channel_stride bytes
 * apart) from every channel's position and advances it modulo the file length, exactly like
 * retrieveIqDataFromBuffer; nothing is written while no file is loaded (as in the reference).
 * Streams: hrfd_play_get_device is asynchronous on the caller's stream (NULL: the handle's own).  Every call hands its
 * kernel the positions of THAT call in a buffer of its own, so calls on different streams may follow each other while
 * earlier kernels are still pending; the positions hrfd_play_get_position reports advance at the call, in call order.
 * hrfd_play_load (and load_file, destroy) free the image: they wait, by themselves, for every kernel that
 * hrfd_play_get_device has launched so far, on whichever stream -- the caller need not synchronise first, but must not
 * call them concurrently with hrfd_play_get_device from another thread (a handle is not thread-safe).
 */
typedef struct hrfd_play hrfd_play;
int hrfd_play_create(uint32_t n_channels, int device, hrfd_play **out);
int hrfd_play_destroy(hrfd_play *h);
int hrfd_play_load_file(hrfd_play *h, const char *path);
int hrfd_play_load(hrfd_play *h, const int8_t *bytes, uint32_t n_bytes);
int hrfd_play_set_position(hrfd_play *h, uint32_t channel, uint32_t byte_index);
int hrfd_play_get_position(hrfd_play *h, uint32_t channel, uint32_t *byte_index);
int hrfd_play_get_device(hrfd_play *h, int8_t *d_out, uint64_t channel_stride,
                         uint32_t bytes_per_channel, void *stream);
int hrfd_play_get(hrfd_play *h, int8_t *out, uint32_t bytes_per_channel);

/* ------------------------------------------------------------------------------
 * Nco (Nco/Nco.cc:186-257, Nco/PhaseAccumulator.cc:157-181): n_channels
 * oscillators advanced `count` samples each; fast != 0 selects runFast's table.
 * i_out/q_out are [n_channels][count] float host buffers.
 * Accuracy: the phase sequence is the reference's bit for bit (float accumulate, double-compare
 * wrap).  fast != 0 (Nco::runFast): the values are the host-built table's -- bit-exact.
 * fast == 0 (Nco::run): the reference calls libm sinf/cosf; the device restates glibc's algorithm
 * (the build hrfd_libm_variant() names) and gives the same floats bit for bit -- the device code is
 * compared with the restatement in C on every float with |x| < 120, in both variants
 * (tests/test_gpu_sincos.py), and that restatement with the host's libm (tests/test_sincos_model.py).
 * The same holds for what is built on Nco::run: the FM modulator and the pm / fm generators.
 *
 * hrfd_nco_create and hrfd_nco_set_frequency REFUSE (HRFD_EINVAL, nothing changed, nothing launched) a
 * frequency whose phase step (float)(2 pi f / fs) is not finite or is 2^24 rad or more in magnitude:
 * the wrap loops subtract 2 pi from a float, which from about 2^27 rad no longer changes it, so the
 * kernel -- like the reference's thread in the same place -- would never return.
 */
typedef struct hrfd_nco hrfd_nco;
int hrfd_nco_create(uint32_t n_channels, float sample_rate, float frequency, int device,
                    hrfd_nco **out);
int hrfd_nco_destroy(hrfd_nco *h);
int hrfd_nco_set_frequency(hrfd_nco *h, uint32_t channel, float frequency);
int hrfd_nco_reset(hrfd_nco *h, uint32_t channel);
int hrfd_nco_run(hrfd_nco *h, int fast, uint32_t count, float *i_out, float *q_out);

/* ------------------------------------------------------------------------------
 * DDC bank: W wideband captures -> C channel streams at 2.048 MS/s (no reference counterpart: the reference tunes one
 * HackRF per station, 64 kHz above it, Radio.cc:1180-1191).  A capture is int8 IQ at R x 2.048 MS/s, R = 1, 2, 4, 8; a
 * call consumes R * out_bytes bytes of every capture and produces out_bytes bytes (even, >= 2) of int8 IQ per channel,
 * the input hrfd_rx takes.  Exact integer arithmetic, the same on every device (tests/ddc_model.py restates it):
 *   N        absolute input-sample counter of the handle (uint64), advanced by R * out_bytes / 2 per call; every capture
 *            keeps its last H = 255 R + 63 samples (zeros after create and reset: silence before the first call)
 *   tuning   channel -> (capture, step, theta_ref, N_ref); sample n is mixed with theta(n) = theta_ref + (n - N_ref) step
 *            mod 2^32 (n < N_ref too).  set_tuning at counter N: theta_ref = theta(N) under the old tuning, N_ref = N,
 *            then the new step: the phase is continuous.  step = round(f / (R 2 048 000) 2^32) mod 2^32 moves +f to DC;
 *            to feed hrfd_rx like the reference's radio, f = station offset + 64 000 (the station lands 64 kHz below
 *            the channel's centre, where upconvertByFsOver4 expects it, Radio.cc:1191)
 *   mixer    k = ((theta + 2^19) >> 20) & 4095, c = COS[k], s = COS[(k - 1024) & 4095], COS[i] = round(32767 cos(2 pi i/4096));
 *            yI = (I c + Q s + 128) >> 8, yQ = (Q c - I s + 128) >> 8 (int16, arithmetic shifts)
 *   stage A  a[m] = sat16((sum_k hA[k] y[m R + R - 1 - k] + 2^14) >> 15), T_A <= 64 taps; T_A = 0: a[m] = y[m R + R - 1]
 *   stage B  b[m] = sat16((sum_k hB[k] a[m - k] + 2^14) >> 15), T_B <= 256 taps; T_B = 0: b = a
 *   output   sat8((b + r) >> (7 - g)), r = g < 7 ? 1 << (6 - g) : 0; g = 0..7 in 6 dB steps (default 0).  A station at
 *            -30 dBFS in the capture stays at -30 dBFS at g = 0; g gives back the bits an int8 stream would lose, and the
 *            squelch's dBFS reading of that channel (hrfd_rx_set_threshold) moves up by 6 g dB with it.
 * Default filters (hrfd_ddc_tables.h, tools/ddc_design.py; hrfd_q15_table "DDC_A2", "DDC_A4", "DDC_A8", "DDC_B", "DDC_COS"):
 * stage A +-220 kHz passband, >= 60 dB from 2.048 MHz - 220 kHz (bypass at R = 1); stage B +-164 kHz, >= 60 dB beyond
 * +-220 kHz.  Both stages refuse tap sets with sum |h| > 65535.  A call applies the filters current at its start to the
 * capture stream, history included.  Arguments are checked before any device is touched (HRFD_EINVAL without a GPU as
 * well); set_tuning / get_phase work on the host's copy of N and never wait for the device: the records and taps a setter
 * changed are copied to the device on the next call's stream, ahead of its launch.  Calls may use different streams:
 * each launch is ordered on the device behind the handle's previous one (the per-capture history is the handle's).
 *   hrfd_ddc_process          host buffers: captures [W][R * out_bytes] -> out [C][out_bytes]; blocking
 *   hrfd_ddc_process_device   device buffers, rows capture_stride / out_stride bytes apart; asynchronous on `stream`
 *                             (a hipStream_t, NULL = the handle's own)
 *   hrfd_ddc_receive          the DDC into a buffer of the handle, [C][n_blocks * block_bytes], then the rx bank on rx's
 *                             stream over it (rx->n_channels == C, the same device): outputs exactly those of
 *                             hrfd_ddc_process_device followed by hrfd_rx_process_block, including the chunks of at most
 *                             64 blocks and the exact replay of channels that failed their speculation (*n_replayed, may
 *                             be NULL).  d_pcm [C][n_blocks][hrfd_rx_pcm_capacity(block_bytes)], d_n_pcm / d_magnitude /
 *                             d_signal_allowed [C][n_blocks] on the device (the last two may be NULL); blocking.
 *
 * The receive key (listen only where someone transmits).  The *_keyed calls take, besides the captures, a key row per
 * channel: uint8 [C][n_keys], rows key_stride bytes apart at any address, n_keys = ceil(M / 2^k) for the M = out_bytes / 2
 * output samples per channel of the call.  k is the handle's key block, 10..17 (hrfd_ddc_set_key_block; default 17: 131072
 * output samples = 262144 bytes = one rx block = 512 PCM samples, the granularity of the spectrum bank's present[b] when it
 * is asked once per block).  Key byte j of a row covers the call-local output samples [j 2^k, (j + 1) 2^k); any non-zero byte
 * is "on":
 *   outk[c][m] = key[c][m >> k] != 0 ? out[c][m] : (0, 0)  (0 <= m < M, call-local; out is what the unkeyed call writes)
 * Everything else a keyed call leaves behind is exactly what the unkeyed call leaves behind: the captures' history, N, and
 * every byte outside the 2 M bytes of each output row.  The key does not touch the handle's state: the DDC carries nothing
 * per channel through time (the history is the capture's, the phase a function of N), so a channel that is keyed on again
 * is at once what it would have been.  A NULL key is the unkeyed call.  The key is read for 0 <= m < M only.
 *   work      the kernel owns one (channel, tile of 1024 outputs) per workgroup; tiles are call-local, so a tile lies in one
 *             key block.  The unit (channel c, tile t) is skipped iff key[c][(1024 t) >> k] == 0.  A skipped unit loads
 *             neither the cosine table nor the taps, nothing of the capture or its history, runs no mixer and no FIR; it
 *             stores the 2 cnt zero bytes of its cnt outputs (the last tile may be short), whatever the row's base address
 *             and stride, and adds 1 to the skip meter of channel c.  The workgroups that keep the captures' history know no
 *             key.
 *   hrfd_ddc_set_key_block    log2 of the key block in output samples, 10..17; from the next call on
 *   hrfd_ddc_n_keys           n_keys of a call of out_bytes under the handle's key block
 *   hrfd_ddc_get_key_skips    waits for the handle's last launch, then reads the units of one channel skipped since create /
 *                             reset (uint64), or their sum over the bank (HRFD_ALL_CHANNELS): the idle share of its work
 *   hrfd_ddc_count_key_skips  host only, no handle: what one call of out_bytes with these key rows (host memory) adds to the
 *                             meters under key block k, counted unit by unit; per_channel [n_channels] may be NULL.  Not
 *                             part of the key's working interface: it is exported so that the tests, and a caller who
 *                             wants to predict the meters, reach the one statement of the skip rule (hrfd_ddc_key.h)
 *   hrfd_ddc_process_keyed    hrfd_ddc_process with key [C][n_keys], dense
 *   hrfd_ddc_process_device_keyed   hrfd_ddc_process_device with d_key, rows key_stride >= n_keys apart
 *   hrfd_ddc_receive_keyed    hrfd_ddc_receive with d_key: outputs exactly those of hrfd_ddc_process_device_keyed followed by
 *                             hrfd_rx_process_block.  The rx bank runs over every channel as in hrfd_ddc_receive: its state
 *                             moves on over a keyed-off block's zeros
 */
typedef struct hrfd_ddc hrfd_ddc;
int hrfd_ddc_create(uint32_t n_captures, uint32_t n_channels, uint32_t decimation, int device, hrfd_ddc **out);
int hrfd_ddc_destroy(hrfd_ddc *d);
int hrfd_ddc_reset(hrfd_ddc *d);              /* history 0, N = 0, every theta_ref = N_ref = 0, skip meters 0 */
int hrfd_ddc_set_tuning(hrfd_ddc *d, uint32_t channel, uint32_t capture, uint32_t step);
int hrfd_ddc_set_gain_shift(hrfd_ddc *d, uint32_t channel, uint32_t g);          /* HRFD_ALL_CHANNELS allowed */
int hrfd_ddc_set_filter(hrfd_ddc *d, int stage, const int16_t *taps, uint32_t n); /* stage 0 = A, 1 = B; n = 0: bypass */
int hrfd_ddc_get_phase(hrfd_ddc *d, uint32_t channel, uint32_t *theta);          /* theta(N) */
int hrfd_ddc_process(hrfd_ddc *d, const int8_t *captures, uint32_t out_bytes, int8_t *out);
int hrfd_ddc_process_device(hrfd_ddc *d, const int8_t *d_captures, uint64_t capture_stride, uint32_t out_bytes,
                            int8_t *d_out, uint64_t out_stride, void *stream);
int hrfd_ddc_receive(hrfd_ddc *d, hrfd_rx *rx, const int8_t *d_captures, uint64_t capture_stride,
                     uint32_t block_bytes, uint32_t n_blocks, uint32_t gain_db, int16_t *d_pcm, uint32_t *d_n_pcm,
                     uint32_t *d_magnitude, uint8_t *d_signal_allowed, uint32_t *n_replayed);
int hrfd_ddc_set_key_block(hrfd_ddc *d, uint32_t log2_samples);                  /* 10..17, default 17 */
int hrfd_ddc_n_keys(hrfd_ddc *d, uint32_t out_bytes, uint32_t *n);
int hrfd_ddc_get_key_skips(hrfd_ddc *d, uint32_t channel, uint64_t *n);          /* HRFD_ALL_CHANNELS: the sum */
int hrfd_ddc_count_key_skips(const uint8_t *key, uint64_t key_stride, uint32_t n_channels, uint32_t out_bytes,
                             uint32_t log2_samples, uint64_t *per_channel, uint64_t *sum);
int hrfd_ddc_process_keyed(hrfd_ddc *d, const int8_t *captures, uint32_t out_bytes, const uint8_t *key, int8_t *out);
int hrfd_ddc_process_device_keyed(hrfd_ddc *d, const int8_t *d_captures, uint64_t capture_stride, uint32_t out_bytes,
                                  const uint8_t *d_key, uint64_t key_stride, int8_t *d_out, uint64_t out_stride, void *stream);
int hrfd_ddc_receive_keyed(hrfd_ddc *d, hrfd_rx *rx, const int8_t *d_captures, uint64_t capture_stride, uint32_t block_bytes,
                           uint32_t n_blocks, const uint8_t *d_key, uint64_t key_stride, uint32_t gain_db, int16_t *d_pcm,
                           uint32_t *d_n_pcm, uint32_t *d_magnitude, uint8_t *d_signal_allowed, uint32_t *n_replayed);

/* ------------------------------------------------------------------------------
 * DUC bank: C channel streams at 2.048 MS/s -> W wideband captures (the DDC's mirror; the reference transmits one station
 * per HackRF, at DC of the stream, Radio.cc:1697-1722).  A channel stream is int8 IQ at 2.048 MS/s, what hrfd_mod_*
 * writes; a call consumes in_bytes bytes (even, >= 2) of every channel and produces R * in_bytes bytes of int8 IQ per
 * capture at R x 2.048 MS/s, R = 1, 2, 4, 8.  Exact integer arithmetic, the same on every device (tests/duc_model.py
 * restates it); m counts channel samples, n = m R + p wideband samples:
 *   N        absolute wideband output-sample counter of the handle (uint64), advanced by R * in_bytes / 2 per call; every
 *            channel keeps its last H = 318 samples (zeros after create and reset: silence before the first call)
 *   tuning   channel -> (capture, step, theta_ref, N_ref); sample n is mixed with theta(n) = theta_ref + (n - N_ref) step
 *            mod 2^32, set_tuning at counter N is phase-continuous, exactly as the DDC's.  step = round(f / (R 2 048 000)
 *            2^32) mod 2^32 puts the channel's DC at +f (no 64 kHz shift: the reference transmits the station at DC)
 *   input    u[m] = x[m] << 8 (x the int8 I or Q)
 *   stage B  b[m] = sat16((sum_k hB[k] u[m - k] + 2^14) >> 15), T_B <= 256 taps, sum |hB| <= 65535; T_B = 0: b = u
 *   amplitude v[m] = (b[m] A + 2^14) >> 15, A = 0..32768 per channel (default 32768: v = b; A = 0 mutes the channel)
 *   stage A  a[n] = sat16((sum_{k : (n - k) mod R = 0} hA[k] v[(n - k) / R] + 2^14) >> 15), the zero-stuffed
 *            interpolation, T_A <= 64 taps, sum |hA[k]| over k = p mod R <= 65535 for every branch p; T_A = 0: a[n] = v[n / R]
 *   mixer    k = ((theta + 2^19) >> 20) & 4095, c = COS[k], s = COS[(k - 1024) & 4095] (the DDC's table), multiplication
 *            by e^{+j theta}: yI = (aI c - aQ s + 2^14) >> 15, yQ = (aQ c + aI s + 2^14) >> 15 (int32, |y| <= 46 341)
 *   sum      S_w[n] = sum of y over the channels mapped to capture w (int32: n_channels <= 32768 cannot overflow it)
 *   output   sat8((S + r) >> s), r = s ? 1 << (s - 1) : 0; s = 0..24 per capture (default 8: one full-scale channel comes
 *            out at full scale).  Every output sample (I and Q counted apart) whose sat8 clipped adds 1 to the capture's
 *            uint64 clip counter (0 after create and reset).
 * Default filters (hrfd_duc_tables.h, tools/duc_design.py; hrfd_q15_table "DUC_A2", "DUC_A4", "DUC_A8"): stage A
 * +-220 kHz passband, >= 60 dB from 2.048 MHz - 220 kHz, DC gain R (hold at R = 1); stage B the DDC's "DDC_B" (+-164 kHz,
 * >= 60 dB beyond +-220 kHz).  A call applies the filters current at its start to the channel streams, history included.
 * Arguments are checked before any device is touched (HRFD_EINVAL without a GPU as well); setters never wait for the
 * device: the records and taps a setter changed are copied to the device on the next call's stream, ahead of its launch.
 * Calls may use different streams: each launch is ordered on the device behind the handle's previous one.
 *   hrfd_duc_process          host buffers: channels [C][in_bytes] -> captures [W][R * in_bytes]; blocking
 *   hrfd_duc_process_device   device buffers, rows channel_stride / capture_stride bytes apart; asynchronous on `stream`
 *                             (a hipStream_t, NULL = the handle's own)
 *   hrfd_duc_transmit         the modulator bank (mod->n_channels == C, the same device) into a buffer of the handle,
 *                             [C][512 * n_per_channel], then the DUC over it, both on `stream`: outputs exactly those of
 *                             hrfd_mod_process_device followed by hrfd_duc_process_device; asynchronous
 *   hrfd_duc_get_clips        waits for the handle's last launch, then reads the capture's clip counter
 *
 * The transmit key (push-to-talk).  The *_keyed calls take, besides the channel streams, a key row per channel: uint8
 * [C][n_keys], rows key_stride bytes apart, n_keys = ceil(M / 2^k) for the M = in_bytes / 2 channel samples of the call.  k
 * is the handle's key block, 10..17 (hrfd_duc_set_key_block; default 17: 131072 channel samples = 262144 bytes = one block
 * of 512 PCM samples, the granularity of the `active` bytes hrfd_tonegen_* and hrfd_afskgen_* write).  Key byte j of a row
 * covers the call-local channel samples [j 2^k, (j + 1) 2^k); any non-zero byte is "on":
 *   xk[c][m] = key[c][m >> k] != 0 ? x[c][m] : 0          (0 <= m < M, call-local)
 * Everything a keyed call leaves behind is exactly what the unkeyed call leaves behind for the input xk: the captures,
 * the clip counters, the H = 318 samples of history for the next call (xk, not x) and N.  An all-zero input is exactly zero
 * at every stage (u = b = v = a = 0, y = (0 + 2^14) >> 15 = 0), so a channel that is keyed off adds nothing to its capture.
 * A NULL key is the unkeyed call.  The bytes of x inside a keyed-off block are not looked at, and the key is read for
 * 0 <= m < M only.  Keying is abrupt, there is no ramp: stage B, the channel filter, confines the splatter of the step to
 * the channel's own +-220 kHz.
 *   work      the kernel owns one (capture, tile of 1024 channel samples) per workgroup and loops over the capture's
 *             channels; tiles are call-local, so a tile lies in one key block.  The unit (channel c, tile t) is skipped, with
 *             none of its loads and none of its arithmetic, iff t >= 1 and key[c][(1024 t) >> k] == 0 and
 *             key[c][(1024 (t - 1)) >> k] == 0 (the tile's look-back lies in the tile in front of it).  The key is tested in
 *             front of the amplitude.  Tile 0 of a call looks back into the history and is always computed.
 *   hrfd_duc_set_key_block    log2 of the key block in channel samples, 10..17; from the next call on, the history stays
 *   hrfd_duc_n_keys           n_keys of a call of in_bytes under the handle's key block
 *   hrfd_duc_get_key_skips    waits for the handle's last launch, then reads the units skipped since create / reset (uint64):
 *                             the idle share of the bank's work
 *   hrfd_duc_process_keyed    hrfd_duc_process with key [C][n_keys], dense
 *   hrfd_duc_process_device_keyed   hrfd_duc_process_device with d_key, rows key_stride >= n_keys apart at any address
 *   hrfd_duc_transmit_keyed   hrfd_duc_transmit with d_key: the modulator bank runs over every channel as in
 *                             hrfd_duc_transmit (its state moves on whether a channel is keyed or not), then the keyed DUC
 */
typedef struct hrfd_duc hrfd_duc;
int hrfd_duc_create(uint32_t n_captures, uint32_t n_channels, uint32_t interpolation, int device, hrfd_duc **out);
int hrfd_duc_destroy(hrfd_duc *d);
int hrfd_duc_reset(hrfd_duc *d);              /* history 0, N = 0, every theta_ref = N_ref = 0, clip and skip counters 0 */
int hrfd_duc_set_tuning(hrfd_duc *d, uint32_t channel, uint32_t capture, uint32_t step);
int hrfd_duc_set_amplitude(hrfd_duc *d, uint32_t channel, uint32_t amplitude);    /* HRFD_ALL_CHANNELS allowed */
int hrfd_duc_set_output_shift(hrfd_duc *d, uint32_t capture, uint32_t s);         /* HRFD_ALL_CHANNELS: every capture */
int hrfd_duc_set_filter(hrfd_duc *d, int stage, const int16_t *taps, uint32_t n); /* stage 0 = A, 1 = B; n = 0: bypass */
int hrfd_duc_get_phase(hrfd_duc *d, uint32_t channel, uint32_t *theta);          /* theta(N) */
int hrfd_duc_get_clips(hrfd_duc *d, uint32_t capture, uint64_t *n);
int hrfd_duc_process(hrfd_duc *d, const int8_t *channels, uint32_t in_bytes, int8_t *captures);
int hrfd_duc_process_device(hrfd_duc *d, const int8_t *d_channels, uint64_t channel_stride, uint32_t in_bytes,
                            int8_t *d_captures, uint64_t capture_stride, void *stream);
int hrfd_duc_transmit(hrfd_duc *d, hrfd_mod *mod, const int16_t *d_pcm, uint32_t n_per_channel, int8_t *d_captures,
                      uint64_t capture_stride, void *stream);
int hrfd_duc_set_key_block(hrfd_duc *d, uint32_t log2_samples);                  /* 10..17, default 17 */
int hrfd_duc_n_keys(hrfd_duc *d, uint32_t in_bytes, uint32_t *n);
int hrfd_duc_get_key_skips(hrfd_duc *d, uint64_t *n);
int hrfd_duc_process_keyed(hrfd_duc *d, const int8_t *channels, uint32_t in_bytes, const uint8_t *key, int8_t *captures);
int hrfd_duc_process_device_keyed(hrfd_duc *d, const int8_t *d_channels, uint64_t channel_stride, uint32_t in_bytes,
                                  const uint8_t *d_key, uint64_t key_stride, int8_t *d_captures, uint64_t capture_stride,
                                  void *stream);
int hrfd_duc_transmit_keyed(hrfd_duc *d, hrfd_mod *mod, const int16_t *d_pcm, uint32_t n_per_channel, const uint8_t *d_key,
                            uint64_t key_stride, int8_t *d_captures, uint64_t capture_stride, void *stream);

/* ------------------------------------------------------------------------------
 * Spectrum bank: W wideband captures -> the power of every FFT bin, and the occupancy of K bands (no reference counterpart
 * in the chain: it stands in for what the reference does by steering the radio, FrequencyScanner::run,
 * FrequencyScanner.cc:378-400, and for the sweep tool beside it, hackrf-tools/hackrf_sweep.c:196-340 -- window, FFT, power
 * per bin).  A capture is int8 IQ at R x 2.048 MS/s, the DDC's input; N = 2^L, L = 8..13.  A call takes n_frames frames
 * (1..65536) of N samples (2 N bytes) from every capture, back to back, no overlap, and is a pure function of its input
 * and the handle's settings: no history, no counter, nothing carried to the next call (unlike SignalTracker there is no
 * tail: a band is present in a call or it is not).  Exact integer arithmetic, the same on every device
 * (tests/spec_model.py restates it); complex values are (re, im) int16, shifts are arithmetic:
 *   window    u = (x w[n] + 128) >> 8 per rail, w an int16 table of N entries, any values (-32768 included): |u| <= 16384
 *             per rail.  Default: round(32767 * 0.5 * (1 - cos(2 pi n / N))) built on the host in double
 *             (hrfd_q15_table "SPEC_HANN_8" .. "SPEC_HANN_13")
 *   transform radix-2 decimation in frequency, L stages in place, natural order in, bit-reversed order out, halving in
 *             every stage, rounded up in the even stages and down in the odd ones (r = 1 - (t mod 2); with one direction
 *             in every stage the halvings' mean of a quarter LSB adds up to a hump of a few LSB around DC).  Stage t = 0..L-1 has span = N >> t, h = span / 2; for every i with (i mod span) < h, the pair
 *             a = z[i], b = z[i + h], twiddle index k = (i mod span) (N / span), c = round(32767 cos(2 pi k / N)),
 *             s = round(32767 sin(2 pi k / N)) (host, double; hrfd_q15_table "SPEC_COS_<L>" / "SPEC_SIN_<L>", N / 2 entries):
 *               z[i]     = (a + b + r) >> 1                                 per component
 *               d        = (a - b + r) >> 1                                 per component
 *               z[i + h] = ((d_re c + d_im s + 2^14) >> 15, (d_im c - d_re s + 2^14) >> 15)
 *             The result is X[k] = z[bitrev_L(k)] ~ DFT(u)[k] / N.  The complex magnitude never grows (<= 23170.5 after the
 *             window), so every component stays within int16 and every product sum within int32.
 *   power     p[k] = re^2 + im^2 (< 2^30) per frame; P[w][k] = the sum over the call's frames, uint64, in natural bin
 *             order k = 0..N-1 (k >= N / 2 are the negative offsets; a bin is R * 2 048 000 / N Hz wide)
 *   bands     K >= 0 bands (at most 65536), band -> (capture, first_bin, n_bins, threshold), 1 <= n_bins <= N, first_bin < N,
 *             bins taken modulo N (a band may wrap through DC or through +-Fs/2), threshold <= 2^44 in power units per
 *             frame (a band cannot hold more: N 2^31).  band_power[b] = the sum of P[capture] over the band's bins (uint64,
 *             < 2^13 2^16 2^30), present[b] = band_power[b] >= threshold * n_frames (<= 2^44 2^16: inside uint64; larger
 *             thresholds and frame counts are refused).  set_band with band == K appends, band < K replaces.
 * Arguments are checked before any device is touched (HRFD_EINVAL without a GPU as well); setters never wait for the
 * device: the window and the bands a setter changed are copied to the device on the next call's stream, ahead of its
 * launch.  Calls may use different streams: each launch is ordered on the device behind the handle's previous one.
 *   hrfd_spec_process         host buffers: captures [W][2 N n_frames] -> power [W][N], band_power [K], present [K] (the
 *                             last two may be NULL when K = 0); blocking
 *   hrfd_spec_process_device  device buffers, capture rows capture_stride bytes apart (any byte address and stride),
 *                             d_power 8-byte aligned; asynchronous on `stream` (a hipStream_t, NULL = the handle's own)
 */
typedef struct hrfd_spec hrfd_spec;
#define HRFD_SPEC_MAX_FRAMES 65536u
#define HRFD_SPEC_MAX_BANDS 65536u
#define HRFD_SPEC_MAX_THRESHOLD (1ull << 44)
int hrfd_spec_create(uint32_t n_captures, uint32_t decimation, uint32_t log2_n, int device, hrfd_spec **out);
int hrfd_spec_destroy(hrfd_spec *s);
int hrfd_spec_set_window(hrfd_spec *s, const int16_t *w);          /* N entries; NULL restores the default */
int hrfd_spec_set_band(hrfd_spec *s, uint32_t band, uint32_t capture, uint32_t first_bin, uint32_t n_bins,
                       uint64_t threshold);
int hrfd_spec_clear_bands(hrfd_spec *s);                           /* K = 0 */
int hrfd_spec_n_bands(hrfd_spec *s, uint32_t *k);
int hrfd_spec_process(hrfd_spec *s, const int8_t *captures, uint32_t n_frames, uint64_t *power, uint64_t *band_power,
                      uint8_t *present);
int hrfd_spec_process_device(hrfd_spec *s, const int8_t *d_captures, uint64_t capture_stride, uint32_t n_frames,
                             uint64_t *d_power, uint64_t *d_band_power, uint8_t *d_present, void *stream);

/* ------------------------------------------------------------------------------
 * Conditioner bank: W wideband captures -> the same captures with the radio's DC offset and IQ imbalance taken out, and
 * the moments a correction is solved from (no reference counterpart: the reference tunes every radio 64 kHz off its
 * station, Radio.cc:1191, and hears one narrow channel, so neither the DC spur nor a station's image reaches it; a
 * wideband capture has both in the band hrfd_spec_* surveys).  A capture is int8 IQ at any rate (the bank does not know
 * R); a call takes n_bytes (even, 2 .. 2^30) from every capture and is a pure function of those bytes and the handle's
 * correction records: no history, no counter, nothing carried to the next call.  Exact integer arithmetic, the same on
 * every device (tests/cal_model.py restates it); shifts are arithmetic:
 *   record    per capture: dc_i, dc_q int32 in Q8 (1/256 LSB), |dc| <= 32512; m_ii, m_iq, m_qi, m_qq int16 in Q14.
 *             Default: identity, dc = 0, m = (16384, 0, 0, 16384).  The setter refuses a row with |m_a| + |m_b| > 32768
 *             (rows (m_ii, m_iq) and (m_qi, m_qq)): with |x| <= 32768 + 32512 = 65280 the int32 sums below then cannot
 *             overflow, 32768 x 65280 + 2^21 < 2^31.
 *   apply     xi = (I << 8) - dc_i, xq = (Q << 8) - dc_q
 *             yi = (m_ii xi + m_iq xq + 2^21) >> 22, yq = (m_qi xi + m_qq xq + 2^21) >> 22; the output is sat8(y).
 *             The identity record returns the input byte for byte (-128 included).  Any matrix inside the row rule is
 *             allowed: the same call injects an imbalance as well as it removes one.
 *   moments   per capture and call eight 64-bit words {n, S_I, S_Q, S_II, S_QQ, S_IQ, clips, 0}: n = n_bytes / 2 and the
 *             sums of I, Q, I^2, Q^2, I Q over the call's RAW INPUT samples (int64, two's complement), clips = the number
 *             of output components (I and Q counted apart) outside -128..127 before sat8, 0 when no output is asked for.
 *             The words of calls add: summing them over about a second, and forgetting old ones, is the caller's policy.
 *   solver    hrfd_cal_solve, host only, no device: IEEE double, only + - x / and sqrt, no fused multiply-add, in this
 *             order (every line one rounding per operation, left to right):
 *               n = (double)moments[0]; mi = S_I / n; mq = S_Q / n
 *               vii = S_II / n - mi mi; vqq = S_QQ / n - mq mq; viq = S_IQ / n - mi mq; D = vii vqq - viq viq
 *               dc = floor(mean 256 + 0.5) clamped to +-32512
 *               r = sqrt(D); m = (16384, 0, floor(((-viq) / r) 16384 + 0.5), floor((vii / r) 16384 + 0.5))
 *             Gram-Schmidt with I as the reference: the corrected capture has equal variances on both rails and no I/Q
 *             correlation.  If n <= 0 (then dc = 0 too), or not vii > 0, or not D > 0, or the row (m_qi, m_qq) breaks the
 *             row rule or leaves int16, m is the identity, dc is kept, and the return value is HRFD_CAL_DEGENERATE (1, not
 *             an error); else HRFD_OK.  Assumption: the capture's content is circular (E[z^2] = 0), which a band of
 *             stations is and one real-valued test tone is not: a capture that holds little but such a tone stays at the
 *             identity.
 * Arguments are checked before any device is touched (HRFD_EINVAL without a GPU as well); setters never wait for the
 * device: the records a setter changed are copied to the device on the next call's stream, ahead of its launch.  Calls may
 * use different streams: each launch is ordered on the device behind the handle's previous one.
 *   hrfd_cal_set_correction   capture: an index or HRFD_ALL_CHANNELS (every capture); dc NULL = (0, 0), m NULL = identity
 *   hrfd_cal_process          host buffers: captures [W][n_bytes] -> out [W][n_bytes] and / or moments [W][8]; either may
 *                             be NULL, not both; blocking
 *   hrfd_cal_process_device   device buffers, rows in_stride / out_stride bytes apart, any byte address and any stride
 *                             >= n_bytes; d_out == d_in with equal strides is allowed (the operation is element-wise), any
 *                             other overlap of the two is refused; d_moments [W][8] 8-byte aligned; d_out or d_moments
 *                             may be NULL, not both; asynchronous on `stream` (a hipStream_t, NULL = the handle's own)
 */
typedef struct hrfd_cal hrfd_cal;
#define HRFD_CAL_MAX_BYTES (1u << 30)
#define HRFD_CAL_MAX_DC 32512
#define HRFD_CAL_MAX_ROW 32768
#define HRFD_CAL_DEGENERATE 1
int hrfd_cal_create(uint32_t n_captures, int device, hrfd_cal **out);
int hrfd_cal_destroy(hrfd_cal *c);
int hrfd_cal_set_correction(hrfd_cal *c, uint32_t capture, const int32_t dc[2], const int16_t m[4]);
int hrfd_cal_get_correction(hrfd_cal *c, uint32_t capture, int32_t dc[2], int16_t m[4]);
int hrfd_cal_process(hrfd_cal *c, const int8_t *captures, uint32_t n_bytes, int8_t *out, int64_t *moments);
int hrfd_cal_process_device(hrfd_cal *c, const int8_t *d_in, uint64_t in_stride, uint32_t n_bytes, int8_t *d_out,
                            uint64_t out_stride, int64_t *d_moments, void *stream);
int hrfd_cal_solve(const int64_t moments[8], int32_t dc[2], int16_t m[4]);

/* ------------------------------------------------------------------------------
 * Tone bank: the PCM of C channels -> per frame the power at K tone frequencies, the frame's energy and a verdict per
 * tone group: which CTCSS sub-tone, which DTMF row and column, whether a pilot is there (no reference counterpart: the
 * reference plays its one channel to a listener; nobody listens to a thousand).  It reads what hrfd_rx_process_device /
 * hrfd_ddc_receive write: PCM rows [C][n_blocks][512] int16 at 8 kS/s and, optionally, n_pcm [C][n_blocks].  A call is a
 * pure function of its input and the handle's settings: no history, no counter, the phase is frame-local.  Exact integer
 * arithmetic, the same on every device (tests/tone_model.py restates it); shifts are arithmetic:
 *   sizes     C = 1..65536 channels; frame length L = 128, 256, .., 8192 (16 ms .. 1.024 s), fixed at create; K = 1..128
 *             tones, one list for every channel; HRFD_TONE_GROUPS = 4 groups; n_blocks = 1..1024 with 512 n_blocks a
 *             multiple of L; F = 512 n_blocks / L frames per channel, back to back without overlap: sample j of a channel
 *             is sample j mod 512 of block j div 512, frame f holds samples f L .. f L + L - 1.
 *   input     x[n] = the int16 sample, or 0 where n_pcm is given and the sample's position in its block is
 *             >= min(n_pcm[c][b], 512): a squelched block (n_pcm = 0) and a short one; the bytes there do not matter.
 *             valid[c][f] = the samples of the frame taken from the input (L when n_pcm is NULL).
 *   window    u[n] = (x[n] w[n] + 2^14) >> 15; w: L int16 entries in -32767..32767 (-32768 is refused, so |u| <= 32767).
 *             Default round(32767 * 0.5 * (1 - cos(2 pi n / L))), host, double: the spectrum bank's formula.
 *   tone k    theta(n) = step_k n mod 2^32, n = 0..L-1 inside the frame; step = round(f / 8000 * 2^32) mod 2^32.  The
 *             mixer indices are the DDC's: i = ((theta + 2^19) >> 20) & 4095, c = COS[i], s = COS[(i - 1024) & 4095], COS
 *             the table behind hrfd_q15_table("DDC_COS").
 *   sums      I_k = sum u[n] c_k[n], Q_k = sum u[n] s_k[n], exact in int64 (|.| < 2^43); I' = (I + 2^14) >> 15, Q' alike
 *             (|.| <= 2^28); P_k = I'^2 + Q'^2 (uint64, < 2^57); E = sum u[n]^2 (uint64, < 2^43).
 *   groups    every tone has a group 0..3 (say DTMF rows 0, DTMF columns 1, CTCSS 2).  Per frame and group: best = the
 *             lowest index among the group's tones with the largest P, 255 for a group without tones (present = 0 then);
 *             present = (valid == L) && (E >= E_min_g) && (P_best >= ((E T_g) >> 8)), T_g a uint32 in Q8, at most 2^20
 *             (E T stays inside uint64), E_min_g <= 2^43.  A pure tone on the frequency gives P / E ~ S1^2 / (2 S2) with
 *             S1 = sum w / 32768, S2 = sum (w / 32768)^2, so T says "the tone holds at least this fraction of the
 *             frame's energy".  Defaults: T_g = 16 L (ratio L / 16: about 0.19 of the energy under the default window),
 *             E_min_g = 256 L.
 * Arguments are checked before any device is touched (HRFD_EINVAL without a GPU as well); a call before any tones are set
 * is refused.  Setters never wait for the device: what a setter changed is copied to the device on the next call's stream,
 * ahead of its launch.  Calls may use different streams: each launch is ordered on the device behind the handle's previous
 * one, so a call chains behind the receive call that filled its input when both are given the same stream.
 *   hrfd_tone_set_tones       K steps and their groups (NULL: all 0); replaces the whole list
 *   hrfd_tone_set_window      L entries; NULL restores the default
 *   hrfd_tone_set_threshold   group: 0..3 or HRFD_ALL_CHANNELS (every group)
 *   hrfd_tone_process         host buffers, dense: pcm [C][n_blocks][512], n_pcm [C][n_blocks] or NULL -> power [C][F][K],
 *                             energy [C][F], valid [C][F], best [C][F][4], present [C][F][4]; any output may be NULL, not
 *                             all; blocking
 *   hrfd_tone_process_device  device buffers; channel rows channel_stride_bytes apart (even, >= 1024 n_blocks), d_pcm at
 *                             any even address; d_n_pcm dense as hrfd_rx_* writes it, or NULL; d_power and d_energy 8-byte
 *                             aligned, d_valid 4-byte aligned; asynchronous on `stream` (a hipStream_t, NULL = the handle's
 *                             own)
 */
typedef struct hrfd_tone hrfd_tone;
#define HRFD_TONE_GROUPS 4
#define HRFD_TONE_MAX_TONES 128
#define HRFD_TONE_MAX_BLOCKS 1024
#define HRFD_TONE_MAX_RATIO (1u << 20)
#define HRFD_TONE_MAX_ENERGY (1ull << 43)
int hrfd_tone_create(uint32_t n_channels, uint32_t frame_len, int device, hrfd_tone **out);
int hrfd_tone_destroy(hrfd_tone *t);
int hrfd_tone_set_tones(hrfd_tone *t, const uint32_t *steps, const uint8_t *groups, uint32_t n_tones);
int hrfd_tone_n_tones(hrfd_tone *t, uint32_t *n_tones);
int hrfd_tone_set_window(hrfd_tone *t, const int16_t *w);
int hrfd_tone_set_threshold(hrfd_tone *t, uint32_t group, uint32_t ratio_q8, uint64_t min_energy);
int hrfd_tone_process(hrfd_tone *t, const int16_t *pcm, const uint32_t *n_pcm, uint32_t n_blocks, uint64_t *power,
                      uint64_t *energy, uint32_t *valid, uint8_t *best, uint8_t *present);
int hrfd_tone_process_device(hrfd_tone *t, const int16_t *d_pcm, uint64_t channel_stride_bytes, const uint32_t *d_n_pcm,
                             uint32_t n_blocks, uint64_t *d_power, uint64_t *d_energy, uint32_t *d_valid, uint8_t *d_best,
                             uint8_t *d_present, void *stream);

/* ------------------------------------------------------------------------------
 * Audio bank: the PCM of C channels -> every channel's audio behind a voice filter and a click-free gate, and M monitor
 * mixes of it: what turns the tone bank's verdicts into something a person or a recorder takes (the reference plays its one
 * channel to a listener; the many-channel counterpart is a mix of the channels that matter).  It reads what
 * hrfd_rx_process_device / hrfd_ddc_receive write and the tone bank reads: PCM rows [C][n_blocks][512] int16 at 8 kS/s and,
 * optionally, n_pcm [C][n_blocks].  Exact integer arithmetic, the same on every device (tests/audio_model.py restates it);
 * shifts are arithmetic:
 *   sizes     C = 1..65536 channels and M = 1..HRFD_AUDIO_MAX_BUSES = 64 buses, fixed at create; T = 1..HRFD_AUDIO_MAX_TAPS =
 *             512 taps, one list for every channel; n_blocks = 1..1024.
 *   input     x[n] = the int16 sample, or 0 where n_pcm is given and the sample's position in its block is
 *             >= min(n_pcm[c][b], 512): the tone bank's law.  The bytes there do not matter, and that includes their way
 *             through the filter's history into the next block and the next call.
 *   filter    h: T int16 taps in Q14 with sum |h| <= 65535 (the bank core's tap check).  acc = sum_k h[k] x[n-k]: |acc| <=
 *             65535 * 32768 < 2^31 - 2^14, exact in int32 at every partial sum.  y[n] = sat16((acc + 2^13) >> 14).  Default
 *             h = {16384}: y = x exactly.  The handle keeps the last T - 1 values of x per channel across calls, zeros after
 *             create and after hrfd_audio_reset, so the outputs of a batch do not depend on how it is cut into calls.
 *             hrfd_audio_set_taps zeroes every channel's history and gate (it acts as a reset of all channels): samples
 *             kept for one filter say nothing under another.
 *   gate      open [C][n_blocks] uint8, 0 = shut, anything else = open; NULL = all open.  p = the gate of the block before,
 *             q = this block's; for a call's first block p is the handle's per-channel prev: 0 after create and reset, else
 *             the q of the previous call's last block.  The envelope of sample n = 0..511 of the block: 32768 q where
 *             p == q; min(32768, 512 (n + 1)) where the gate opens; max(0, 32768 - 512 (n + 1)) where it shuts: a ramp of
 *             64 samples (8 ms), no clicks.  z[n] = (y[n] e[n] + 2^14) >> 15: y exactly at e = 32768, 0 at e = 0.
 *   squelch   hrfd_audio_gate* fills `open` from the tone bank's best / present [C][F][4] (F = 512 n_blocks / frame_len;
 *             frame_len a power of two in 128..8192 with 512 n_blocks a multiple of it, group 0..3): stateless but for
 *             want[c], a tone index 0..127, HRFD_AUDIO_ANY_TONE or HRFD_AUDIO_NO_TONE (always open; the default).  Frame f
 *             matches when present[c][f][group] != 0 && (want == ANY || best[c][f][group] == want).  Block b is open when
 *             want == NO_TONE, or when any frame that overlaps it matches: frames b 512 / L .. (b + 1) 512 / L - 1 for
 *             L <= 512, the frame b 512 / L (rounded down) for L > 512.  Hang time and debouncing are the caller's policy
 *             on this per-block gate; a caller with a gate of their own passes their own array to the process call.
 *   buses     bus m holds a list of N_m <= HRFD_AUDIO_MAX_LIST = 4096 entries, each a channel and a gain: int16 in Q12,
 *             -32767..32767 (-32768 is refused).  A channel may be on many buses and several times on one.
 *             s[n] = sum_j g_j z_{c_j}[n], exact in int64 (|s| < 2^42); mix[m][n] = sat16((s + 2^11) >> 12); clips[m] = the
 *             samples of this call whose saturation changed the value (written, not accumulated).  An empty bus gives
 *             zeros and 0 clips.
 * Arguments are checked before any device is touched (HRFD_EINVAL without a GPU as well).  Setters never wait for the
 * device: what a setter changed is copied to the device on the next call's stream, ahead of its launch.  Calls may use
 * different streams: each launch is ordered on the device behind the handle's previous one (the history and prev are the
 * handle's), so a call chains behind the receive and tone calls that filled its input when all are given the same stream.
 *   hrfd_audio_set_taps        T taps; zeroes every channel's history and prev
 *   hrfd_audio_set_bus         replaces bus's whole list; n = 0 clears it
 *   hrfd_audio_set_want        channel: 0..C-1 or HRFD_ALL_CHANNELS
 *   hrfd_audio_reset           history and prev of one channel, or of all (HRFD_ALL_CHANNELS), from the next call on
 *   hrfd_audio_gate            host buffers: best, present [C][F][4] -> open [C][n_blocks]; blocking
 *   hrfd_audio_gate_device     device buffers; asynchronous on `stream` (a hipStream_t, NULL = the handle's own)
 *   hrfd_audio_process         host buffers, dense: pcm [C][n_blocks][512], n_pcm and open [C][n_blocks] or NULL -> out
 *                              [C][n_blocks][512] (z), mix [M][n_blocks][512], clips [M]; any output may be NULL, but not
 *                              both out and mix; blocking
 *   hrfd_audio_process_device  device buffers; input rows channel_stride_bytes apart, rows of d_out out_stride_bytes apart
 *                              (both even and >= 1024 n_blocks), d_pcm, d_out and d_mix at any even address, d_clips 4-byte
 *                              aligned; d_mix dense.  Without d_out, z lives in a buffer of the handle's.  A d_out that
 *                              overlaps the input is refused: a block needs the raw tail of the block before it.
 *                              Asynchronous on `stream`
 */
typedef struct hrfd_audio hrfd_audio;
#define HRFD_AUDIO_MAX_BUSES 64
#define HRFD_AUDIO_MAX_TAPS 512
#define HRFD_AUDIO_MAX_LIST 4096
#define HRFD_AUDIO_MAX_BLOCKS 1024
#define HRFD_AUDIO_ANY_TONE 254
#define HRFD_AUDIO_NO_TONE 255
int hrfd_audio_create(uint32_t n_channels, uint32_t n_buses, int device, hrfd_audio **out);
int hrfd_audio_destroy(hrfd_audio *a);
int hrfd_audio_set_taps(hrfd_audio *a, const int16_t *taps, uint32_t n);
int hrfd_audio_set_bus(hrfd_audio *a, uint32_t bus, const uint32_t *channels, const int16_t *gains, uint32_t n);
int hrfd_audio_set_want(hrfd_audio *a, uint32_t channel, uint32_t want);
int hrfd_audio_reset(hrfd_audio *a, uint32_t channel);
int hrfd_audio_gate(hrfd_audio *a, const uint8_t *best, const uint8_t *present, uint32_t frame_len, uint32_t group,
                    uint32_t n_blocks, uint8_t *open);
int hrfd_audio_gate_device(hrfd_audio *a, const uint8_t *d_best, const uint8_t *d_present, uint32_t frame_len, uint32_t group,
                           uint32_t n_blocks, uint8_t *d_open, void *stream);
int hrfd_audio_process(hrfd_audio *a, const int16_t *pcm, const uint32_t *n_pcm, const uint8_t *open, uint32_t n_blocks,
                       int16_t *out, int16_t *mix, uint32_t *clips);
int hrfd_audio_process_device(hrfd_audio *a, const int16_t *d_pcm, uint64_t channel_stride_bytes, const uint32_t *d_n_pcm,
                              const uint8_t *d_open, uint32_t n_blocks, int16_t *d_out, uint64_t out_stride_bytes, int16_t *d_mix,
                              uint32_t *d_clips, void *stream);

/* ------------------------------------------------------------------------------
 * Resampler bank: the PCM of C channels at one rate -> the same audio at L / M times that rate: what stands between the
 * library's 8 kS/s (the PCM hrfd_rx_process_device / hrfd_ddc_receive write, the audio bank's out and mix rows, the PCM
 * hrfd_mod / hrfd_duc_transmit read) and the 48, 44.1 or 16 kS/s of sound cards, recorders and codecs.  A rational polyphase
 * FIR, the same for every channel of a handle.  Exact integer arithmetic, the same on every device and however a stream is
 * cut into calls (tests/resamp_model.py restates it); shifts are arithmetic, div and mod are those of non-negative integers:
 *   sizes     C = 1..65536 channels, L = up and M = down in 1..HRFD_RESAMP_MAX_RATIO = 512 with gcd(L, M) = 1 and M <= 8 L,
 *             all fixed at create.  T = 1..HRFD_RESAMP_MAX_TAPS = 16384 taps with K = ceil(T / L) <=
 *             HRFD_RESAMP_MAX_BRANCH = 512 taps per branch.  Per call n_in = 1..HRFD_RESAMP_MAX_IN = 524288 samples per
 *             channel with n_in L < 2^31.  Everything else is refused with HRFD_EINVAL and a text that names the rule.
 *   taps      h: T int16 in Q14 at the rate L times the input's, h[k] = 0 for k >= T; one list for every channel.  Branch p
 *             = 0..L-1 holds h[p], h[p + L], ..: sum_k |h[p + k L]| <= 65535 for every branch (the bank core's tap check).
 *             With it |acc| <= 65535 * 32768 < 2^31 - 2^13: int32 is exact at every partial sum and under the rounding
 *             constant.  A handle with L = M = 1 starts with {16384}, the identity; any other handle refuses the process
 *             calls with HRFD_ESTATE until hrfd_resamp_set_taps has been called.  hrfd_resamp_set_taps acts as
 *             hrfd_resamp_reset(HRFD_ALL_CHANNELS): samples kept for one filter say nothing under another.
 *   time      the handle (not the channel) keeps one integer d, 0 <= d < M: 0 after create, after hrfd_resamp_set_taps and
 *             after hrfd_resamp_reset(HRFD_ALL_CHANNELS).  A call of n_in samples gives n_out = 0 if n_in L <= d, else
 *             ceil((n_in L - d) / M) outputs per channel, the same count for every channel.  Output j = 0..n_out-1 has
 *             q = d + j M, i = q div L, p = q mod L and
 *                 y[j] = sat16((sum_{k=0}^{K-1} h[p + k L] x[i - k] + 2^13) >> 14)
 *             where x[0..n_in-1] is the call's input and x[-1], x[-2], .. are the channel's history: the last K - 1 inputs
 *             of the calls before, zeros after create and reset.  Afterwards d += n_out M - n_in L, again in 0..M-1.  d
 *             lives on the host (every n_in is known there), so no call waits for the device.  A call may give no output
 *             (L = 1, M = 6, n_in = 1 with d > 0): it is valid, moves the history and returns n_out = 0.
 *             hrfd_resamp_reset(channel) zeroes that channel's history only; d goes on.
 *   input     rows of n_in int16, channel_stride_bytes apart (even, >= 2 n_in), at even addresses.  n_pcm [C][n_in / 512]
 *             is optional and accepted only when n_in is a multiple of 512: then x = 0 where a sample's position in its
 *             block of 512 is >= min(n_pcm[c][b], 512), the tone and audio banks' law; the bytes there do not matter, and
 *             that includes their way through the history into the next call.  So the bank takes the receive chain's PCM
 *             and n_pcm directly, the audio bank's out, or its mix rows (C = the number of buses).
 *   output    rows of n_out int16, out_stride_bytes apart (even, >= 2 out_capacity), at any even address.  out_capacity is
 *             what a row can take, in samples: a call whose n_out is larger is refused with HRFD_EINVAL before anything is
 *             launched or any state moves.  *n_out is what the call produced; hrfd_resamp_out_count says beforehand what
 *             the next call of n_in samples would produce.  Samples n_out..out_capacity-1 of a row are left as they were.
 *             An out that overlaps the input is refused: other workgroups of the launch still read it.
 * Arguments are checked before any device is touched (HRFD_EINVAL without a GPU as well).  Setters never wait for the
 * device: what a setter changed is copied to the device on the next call's stream, ahead of its launch.  Calls may use
 * different streams: each launch is ordered on the device behind the handle's previous one (the history is the handle's), so
 * a call chains behind the audio call that filled its input when both are given the same stream.
 *   hrfd_resamp_create          up = L, down = M
 *   hrfd_resamp_set_taps        T taps; zeroes every channel's history and d
 *   hrfd_resamp_reset           the history of one channel, or the histories of all and d (HRFD_ALL_CHANNELS), from the next
 *                               call on
 *   hrfd_resamp_out_count       the n_out of the next call, if it takes n_in samples
 *   hrfd_resamp_process         host buffers, dense: pcm [C][n_in], n_pcm [C][n_in / 512] or NULL -> out, rows of
 *                               out_capacity samples of which the first *n_out are written; blocking
 *   hrfd_resamp_process_device  device buffers; asynchronous on `stream` (a hipStream_t, NULL = the handle's own); *n_out is
 *                               host memory and valid on return
 */
typedef struct hrfd_resamp hrfd_resamp;
#define HRFD_RESAMP_MAX_RATIO 512
#define HRFD_RESAMP_MAX_TAPS 16384
#define HRFD_RESAMP_MAX_BRANCH 512
#define HRFD_RESAMP_MAX_IN 524288
int hrfd_resamp_create(uint32_t n_channels, uint32_t up, uint32_t down, int device, hrfd_resamp **out);
int hrfd_resamp_destroy(hrfd_resamp *r);
int hrfd_resamp_set_taps(hrfd_resamp *r, const int16_t *taps, uint32_t n);
int hrfd_resamp_reset(hrfd_resamp *r, uint32_t channel);
int hrfd_resamp_out_count(hrfd_resamp *r, uint32_t n_in, uint32_t *n_out);
int hrfd_resamp_process(hrfd_resamp *r, const int16_t *pcm, const uint32_t *n_pcm, uint32_t n_in, int16_t *out,
                        uint32_t out_capacity, uint32_t *n_out);
int hrfd_resamp_process_device(hrfd_resamp *r, const int16_t *d_pcm, uint64_t channel_stride_bytes, const uint32_t *d_n_pcm,
                               uint32_t n_in, int16_t *d_out, uint64_t out_stride_bytes, uint32_t out_capacity, uint32_t *n_out,
                               void *stream);

/* ------------------------------------------------------------------------------
 * Level bank: the PCM of C channels -> the same audio at an even loudness: a per-channel automatic gain control.  Behind a
 * DDC bank the AM and SSB demodulators give PCM in proportion to each station's strength, and the radio's one hardware gain
 * cannot even them out; this bank does, on the audio.  It reads what hrfd_rx_process_device / hrfd_ddc_receive write and the
 * tone and audio banks read: PCM rows [C][n_blocks][512] int16 at 8 kS/s and, optionally, n_pcm [C][n_blocks].  Exact integer
 * arithmetic with a law of its own, the same on every device and however a stream is cut into calls (tests/level_model.py
 * restates it); shifts are arithmetic, the division is that of non-negative integers.  Everything is per channel; a frame
 * is HRFD_LEVEL_FRAME = 64 samples (8 ms), a block 8 frames:
 *   sizes     C = 1..65536 channels, fixed at create; W = 1..HRFD_LEVEL_MAX_WEIGHTS = 64 release weights, one table for
 *             every channel; n_blocks = 1..HRFD_LEVEL_MAX_BLOCKS = 1024.
 *   input     x[n] = the int16 sample, or 0 where n_pcm is given and the sample's position in its block is
 *             >= min(n_pcm[c][b], 512): the tone bank's law.  The bytes there do not matter.
 *   peak      p[f] = max |x| over frame f, 0..32768 (|-32768| = 32768).  Frames before the stream's start and after
 *             hrfd_level_reset have p = 0.
 *   envelope  E[f] = max(floor, max_{k=0..W-1} ((p[f-k] w[k] + 2^14) >> 15)).  w: Q15 weights with w[0] = 32768 (required:
 *             E[f] >= p[f] rests on it) and every w[k] <= 32768.  A weighted sliding maximum: it rises within the frame and
 *             falls as the table says (hang time, then decay); there is no recurrence.
 *   gain      g[f] = (target << 12) / E[f], Q12.  target = 0..32767, floor = 16..32768, per channel: g <= 8388352 < 2^23,
 *             and the largest gain is target / floor.
 *   ramp      sample n = 0..63 of frame f has gs = g[f] where g[f] <= g[f-1] (attack takes effect at the frame boundary),
 *             else g[f-1] + (((g[f] - g[f-1]) (n + 1)) >> 6) (release is ramped over the frame).  g[f-1] of a call's first
 *             frame is recomputed by the gain rule from the 64 peaks before it under the settings of THIS call: the handle's
 *             whole state is the last 64 peaks per channel.
 *   output    y = (x gs + 2^11) >> 12.  |x| <= p[f] <= E[f] and gs <= g[f] give |x gs| <= target << 12 < 2^27, so
 *             |y| <= target always: no saturation, no clip counter.
 *   bypass    per channel: y = x (0 behind the block's limit); gain and peak are reported as if not bypassed.
 *   defaults  target 8192, floor 64, no bypass; W = 64 with w[k] = 32768 for k < 8 and (32768 (64 - k)) / 56 from there: a
 *             64 ms hang, then linear to the end of a 512 ms window.
 * hrfd_level_set_weights and hrfd_level_set do not clear the peaks (they are facts about the signal); only hrfd_level_reset
 * does.  Arguments are checked before any device is touched (HRFD_EINVAL without a GPU as well).  Setters never wait for the
 * device: what a setter changed is copied to the device on the next call's stream, ahead of its launch.  Calls may use
 * different streams: each launch is ordered on the device behind the handle's previous one (the peaks are the handle's), so
 * a call chains behind the receive call that filled its input when both are given the same stream.
 *   hrfd_level_set_weights     W weights, w[0] = 32768; keeps the peaks
 *   hrfd_level_set             channel: 0..C-1 or HRFD_ALL_CHANNELS; keeps the peaks
 *   hrfd_level_set_bypass      channel: 0..C-1 or HRFD_ALL_CHANNELS; on: 0 = levelled, anything else = bypassed
 *   hrfd_level_reset           the peaks of one channel, or of all (HRFD_ALL_CHANNELS), from the next call on
 *   hrfd_level_process         host buffers, dense: pcm [C][n_blocks][512], n_pcm [C][n_blocks] or NULL -> out
 *                              [C][n_blocks][512] (y), gain uint32 [C][8 n_blocks] (g[f]), peak uint16 [C][8 n_blocks]
 *                              (p[f]: a VU meter, and what a caller derives the tone bank's min_energy from); any output may
 *                              be NULL, but not all three: without out the call is a meter.  out may be pcm itself; blocking
 *   hrfd_level_process_device  device buffers; input rows channel_stride_bytes apart, rows of d_out out_stride_bytes apart
 *                              (both even and >= 1024 n_blocks), d_pcm, d_out and d_peak at any even address, d_n_pcm and
 *                              d_gain 4-byte aligned; d_gain and d_peak dense.  In place is allowed: d_out at exactly the
 *                              input's address with the same stride, where every sample is read by the lane that overwrites
 *                              it.  Any other overlap of d_out and the input is refused.  Asynchronous on `stream` (a
 *                              hipStream_t, NULL = the handle's own)
 */
typedef struct hrfd_level hrfd_level;
#define HRFD_LEVEL_FRAME 64
#define HRFD_LEVEL_MAX_WEIGHTS 64
#define HRFD_LEVEL_MAX_BLOCKS 1024
int hrfd_level_create(uint32_t n_channels, int device, hrfd_level **out);
int hrfd_level_destroy(hrfd_level *l);
int hrfd_level_set_weights(hrfd_level *l, const uint16_t *w, uint32_t n);
int hrfd_level_set(hrfd_level *l, uint32_t channel, uint32_t target, uint32_t floor);
int hrfd_level_set_bypass(hrfd_level *l, uint32_t channel, int on);
int hrfd_level_reset(hrfd_level *l, uint32_t channel);
int hrfd_level_process(hrfd_level *l, const int16_t *pcm, const uint32_t *n_pcm, uint32_t n_blocks, int16_t *out, uint32_t *gain,
                       uint16_t *peak);
int hrfd_level_process_device(hrfd_level *l, const int16_t *d_pcm, uint64_t channel_stride_bytes, const uint32_t *d_n_pcm,
                              uint32_t n_blocks, int16_t *d_out, uint64_t out_stride_bytes, uint32_t *d_gain, uint16_t *d_peak,
                              void *stream);

/* ------------------------------------------------------------------------------
 * DCS bank: digital coded squelch ("DPL") decoded on the PCM of C channels, the digital sibling of the tone bank's CTCSS.  It
 * reads what hrfd_rx_process_device / hrfd_ddc_receive write: PCM rows [C][n_blocks][512] int16 at 8 kS/s and, optionally,
 * n_pcm [C][n_blocks].  A DCS word is 23 bits sent cyclically at 134.4 bit/s, 8000 / 134.4 = 1250 / 21 samples a bit, and a
 * transmitter's clock stays within a small part of a bit over the 171 ms of a word: so the bank recovers no clock.  The word
 * that ends at sample m is 23 slicer bits on a fixed grid behind m, every sample has one, and a block's verdict is a count of
 * samples.  Exact integer arithmetic without a recurrence or a tolerance, the same on every device and however a stream is
 * cut into calls (tests/dcs_model.py restates it).  Everything is per channel:
 *   sizes     C = 1..65536 channels, fixed at create; T = 1..HRFD_DCS_MAX_TAPS = 512 taps and K = 0..HRFD_DCS_MAX_CODES = 128
 *             list entries, one list of each for the bank; n_blocks = 1..HRFD_DCS_MAX_BLOCKS = 1024.
 *   input     x[m] = sample m of the channel's stream, or 0 where n_pcm is given and the sample's position in its block is
 *             >= min(n_pcm[c][b], 512) (the level bank's rule; stream time advances 512 a block regardless), and 0 before
 *             the stream's start or behind hrfd_dcs_reset.
 *   slicer    acc[m] = sum_{j<T} h[j] x[m-j], h int16 in Q14 with sum |h| <= 65535, so acc is exact in int32;
 *             s[m] = 1 if acc[m] > 0, else 0.  No rounding, no hysteresis.  A new handle has the single tap 16384.
 *   word      D[k] = floor(1250 k / 21), k = 0..22 (D[0] = 0, D[22] = 1309); w[m] = sum_k s[m - D[k]] << (22 - k): the
 *             newest bit is bit 22.  DCS sends bit 0 first, so an aligned window reads the word as written.
 *   canonical c[m] = the least of the 23 rotations of w[m] within 23 bits.  The (23,12) Golay code is cyclic: every sample
 *             phase sees a rotation of the word sent, and this step removes the phase.
 *   codes     word(code), code = 0..511 (three octal digits), = (p << 12) | 0x800 | code, p the 11-bit remainder of
 *             (0x800 | code) x^11 modulo g = 0xC75 (bit i = x^i): word(023) = 0x763813.  An inverted code is the complement
 *             in 23 bits.  Entries with one canonical word are aliases (023 = 340 = 766; D023I = D047N): a list that holds
 *             two is refused, so a sample matches at most one entry.
 *   hits      hits[b][k] = the number of the 512 positions m of block b with c[m] == canonical(entry k), 0..512.
 *   verdict   best[b][g] = the entry of group g (0..3) with the most hits, the lowest index on a tie, also when all are 0;
 *             present[b][g] = hits[b][best] >= min_hits[g], min_hits = 1..512 per group, 128 unless set.  A group without
 *             entries has best HRFD_DCS_NO_BEST = 255 and present 0, as in the tone bank.  best and present are laid out
 *             [C][n_blocks][4] uint8, the tone bank's at frame_len = 512: hrfd_audio_gate / hrfd_audio_gate_device take them
 *             unchanged, with `want` an index into the code list.
 *   state     per channel the last 512 inputs and the last 1312 slicer bits (1309 are read); read at a call's start,
 *             replaced at its end.  A stream cut into calls anywhere on block boundaries gives the outputs of one call.
 * Left out: bit-error tolerance, detecting the 134.4 Hz turn-off code, per-channel lists, DC removal beyond what the taps do,
 * debouncing over blocks.  The generator is the bank below, hrfd_dcsgen_* (DESIGN.md 3.20).
 * Arguments are checked before any device is touched (HRFD_EINVAL without a GPU as well).  Setters never wait for the device:
 * what a setter changed is copied to the device on the next call's stream, ahead of its launch.  Calls may use different
 * streams: each launch is ordered on the device behind the handle's previous one.
 *   hrfd_dcs_set_taps        T taps; zeroes every channel's state (as hrfd_audio_set_taps)
 *   hrfd_dcs_set_codes       the whole list: codes [n], inverted [n] (0 / not 0) or NULL (none), groups [n] (0..3) or NULL (all
 *                            0); n = 0 clears it.  Keeps the state: the slicer bits are facts about the signal
 *   hrfd_dcs_n_codes         K
 *   hrfd_dcs_set_min_hits    group: 0..3 or HRFD_ALL_CHANNELS (every group); n = 1..512
 *   hrfd_dcs_reset           the state of one channel, or of all (HRFD_ALL_CHANNELS), from the next call on
 *   hrfd_dcs_process         host buffers, dense: pcm [C][n_blocks][512], n_pcm [C][n_blocks] or NULL -> hits uint16
 *                            [C][n_blocks][K], best and present uint8 [C][n_blocks][4]; any output may be NULL, but not all
 *                            three; blocking
 *   hrfd_dcs_process_device  device buffers; input rows channel_stride_bytes apart (even and >= 1024 n_blocks), d_pcm and
 *                            d_hits at any even address, d_n_pcm 4-byte aligned, the outputs dense.  Asynchronous on `stream`
 *                            (a hipStream_t, NULL = the handle's own)
 *   hrfd_dcs_code_word       on the host: word(code), complemented where inverted != 0, and its canonical word; either
 *                            result may be NULL, not both
 */
typedef struct hrfd_dcs hrfd_dcs;
#define HRFD_DCS_MAX_TAPS 512
#define HRFD_DCS_MAX_CODES 128
#define HRFD_DCS_MAX_BLOCKS 1024
#define HRFD_DCS_GROUPS 4
#define HRFD_DCS_NO_BEST 255
int hrfd_dcs_create(uint32_t n_channels, int device, hrfd_dcs **out);
int hrfd_dcs_destroy(hrfd_dcs *d);
int hrfd_dcs_set_taps(hrfd_dcs *d, const int16_t *taps, uint32_t n);
int hrfd_dcs_set_codes(hrfd_dcs *d, const uint16_t *codes, const uint8_t *inverted, const uint8_t *groups, uint32_t n);
int hrfd_dcs_n_codes(hrfd_dcs *d, uint32_t *n);
int hrfd_dcs_set_min_hits(hrfd_dcs *d, uint32_t group, uint32_t n);
int hrfd_dcs_reset(hrfd_dcs *d, uint32_t channel);
int hrfd_dcs_process(hrfd_dcs *d, const int16_t *pcm, const uint32_t *n_pcm, uint32_t n_blocks, uint16_t *hits, uint8_t *best,
                     uint8_t *present);
int hrfd_dcs_process_device(hrfd_dcs *d, const int16_t *d_pcm, uint64_t channel_stride_bytes, const uint32_t *d_n_pcm,
                            uint32_t n_blocks, uint16_t *d_hits, uint8_t *d_best, uint8_t *d_present, void *stream);
int hrfd_dcs_code_word(uint32_t code, int inverted, uint32_t *word, uint32_t *canonical);

/* ------------------------------------------------------------------------------
 * Tone generator bank: signalling on the PCM of C transmit channels: CTCSS sub-tones, DTMF digits, tone bursts and paging
 * sequences, added to the rows that hrfd_mod_* and hrfd_duc_transmit read.  The mirror of the tone bank: it sends on the
 * detector's own phase grid.  PCM rows [C][n_blocks][512] int16 at 8 kS/s; there is no n_pcm (transmit PCM has none), and
 * every sample of every block is written.  Exact integer arithmetic, the same on every device (tests/tonegen_model.py
 * restates it); shifts are arithmetic.  Everything is per channel:
 *   sizes     C = 1..65536 channels, fixed at create; n_blocks = 1..HRFD_TONEGEN_MAX_BLOCKS = 1024; HRFD_TONEGEN_TRACKS = 2
 *             tracks per channel; at most HRFD_TONEGEN_MAX_SEGMENTS = 32 segments per track and channel that have not ended.
 *   time      the handle keeps one uint64 sample counter N, the stream time of the next call's first sample.  Every call
 *             advances it by 512 n_blocks, on the host.  Every stream time stays below 2^63.
 *   segment   {gap, length, step_a, step_b, amp_a, amp_b}, six uint32, with a start s (uint64 stream time).  step =
 *             round(f / 8000 * 2^32), the tone bank's; amp = 0..32767; length = 1..2^32-2 samples, or HRFD_TONEGEN_FOREVER =
 *             0xFFFFFFFF: no end.  On one track segments never overlap; segments on different tracks may.
 *   law       of one segment at stream time n, k = n - s, 0 <= k < length:
 *               theta_x = (step_x k) mod 2^32             (only the low 32 bits of k matter)
 *               i_x = ((theta_x + 2^19) >> 20) & 4095
 *               S_x = COS[(i_x - 1024) & 4095]            (COS: "DDC_COS"; the tone bank's sine index: every segment starts at
 *                                                          a zero crossing)
 *               v = (amp_a S_a + amp_b S_b + 2^14) >> 15  (fits int32: 2 x 32767^2 + 2^14 < 2^31)
 *               e = min(k + 1, length - k, 64)            (FOREVER: min(k + 1, 64))
 *               g = (v e + 32) >> 6
 *             a linear ramp of 64 samples (8 ms) at both ends, g = v between them.
 *   output    y = sat16(x + g_track0 + g_track1); x is the input sample, or 0 when the call has no input (generate only).
 *             clips[c] counts the samples where the saturation changed the value, until hrfd_tonegen_reset.
 *   active    optional uint8 [C][n_blocks]: bit t is set when a segment of track t overlaps the block.  A caller keys a
 *             transmitter with it.
 * The output at stream time n is a pure function of n, the queue and x: however a stream is cut into calls, it comes out the
 * same.  Segments that have ended (end <= N) leave the queue with the next call, hrfd_tonegen_queue or hrfd_tonegen_cut.
 * Arguments are checked before any device is touched (HRFD_EINVAL without a GPU as well).  No setter waits for the device:
 * what changed is copied to the device on the next call's stream, ahead of its launch, and a call that already runs keeps the
 * queue it was launched with.  Calls may use different streams: each launch is ordered on the device behind the handle's
 * previous one.
 *   hrfd_tonegen_queue          n = 1..32 segments on one track of one channel, or of all (HRFD_ALL_CHANNELS).  The first begins
 *                               at start + segs[0].gap, each next one gap behind the end of the one before.  start =
 *                               HRFD_TONEGEN_APPEND: max(N, the end of the track's last segment), per channel.  Segments may
 *                               be queued in front of or between those already there.  Refused whole (HRFD_EINVAL, nothing
 *                               queued on any channel): a start before N, an overlap on the track, anything behind a FOREVER
 *                               segment, more than 32 segments that have not ended, an amp above 32767, a length of 0, a
 *                               time at or above 2^63
 *   hrfd_tonegen_cut            one track of one channel, or of all: the segment in progress at N (s <= N < end) is trimmed
 *                               to end at min(its end, N + 64), which under the law is a ramp down; those not yet begun are
 *                               dropped
 *   hrfd_tonegen_reset          empties every queue, N = 0, clips = 0
 *   hrfd_tonegen_set_time       moves the clock only: the queues stay (a segment the clock jumps into goes on at its k)
 *   hrfd_tonegen_time           N
 *   hrfd_tonegen_pending        of one track of one channel: the segments that have not ended at N, and the end of the last
 *                               of them (N where there is none, UINT64_MAX behind a FOREVER segment); either result may be
 *                               NULL, not both
 *   hrfd_tonegen_get_clips      clips[channel]; blocks until the handle's calls have run
 *   hrfd_tonegen_process        host buffers, dense: pcm [C][n_blocks][512] or NULL (generate only) -> out [C][n_blocks][512],
 *                               active [C][n_blocks] or NULL.  out may be pcm itself; blocking
 *   hrfd_tonegen_process_device device buffers; input rows channel_stride_bytes apart, rows of d_out out_stride_bytes apart
 *                               (both even and >= 1024 n_blocks), d_pcm and d_out at any even address, d_active dense.  d_pcm
 *                               may be NULL (generate only; its stride is not looked at).  In place is allowed: d_out at exactly
 *                               the input's address with the same stride; a block no segment touches is then neither read
 *                               nor written.  Any other overlap of d_out and the input is refused.  Asynchronous on `stream`
 *                               (a hipStream_t, NULL = the handle's own)
 */
typedef struct hrfd_tonegen hrfd_tonegen;
typedef struct hrfd_tonegen_segment
{
  uint32_t gap;                            /* samples of silence in front of the segment */
  uint32_t length;                         /* samples, or HRFD_TONEGEN_FOREVER */
  uint32_t step_a, step_b;
  uint32_t amp_a, amp_b;
} hrfd_tonegen_segment;
#define HRFD_TONEGEN_TRACKS 2
#define HRFD_TONEGEN_MAX_SEGMENTS 32
#define HRFD_TONEGEN_MAX_BLOCKS 1024
#define HRFD_TONEGEN_FOREVER 0xffffffffu
#define HRFD_TONEGEN_APPEND UINT64_MAX
int hrfd_tonegen_create(uint32_t n_channels, int device, hrfd_tonegen **out);
int hrfd_tonegen_destroy(hrfd_tonegen *t);
int hrfd_tonegen_queue(hrfd_tonegen *t, uint32_t channel, uint32_t track, const hrfd_tonegen_segment *segs, uint32_t n,
                       uint64_t start);
int hrfd_tonegen_cut(hrfd_tonegen *t, uint32_t channel, uint32_t track);
int hrfd_tonegen_reset(hrfd_tonegen *t);
int hrfd_tonegen_set_time(hrfd_tonegen *t, uint64_t N);
int hrfd_tonegen_time(hrfd_tonegen *t, uint64_t *N);
int hrfd_tonegen_pending(hrfd_tonegen *t, uint32_t channel, uint32_t track, uint32_t *n_segments, uint64_t *end);
int hrfd_tonegen_get_clips(hrfd_tonegen *t, uint32_t channel, uint64_t *n);
int hrfd_tonegen_process(hrfd_tonegen *t, const int16_t *pcm, uint32_t n_blocks, int16_t *out, uint8_t *active);
int hrfd_tonegen_process_device(hrfd_tonegen *t, const int16_t *d_pcm, uint64_t channel_stride_bytes, uint32_t n_blocks,
                                int16_t *d_out, uint64_t out_stride_bytes, uint8_t *d_active, void *stream);

/* ------------------------------------------------------------------------------
 * DCS generator bank: digital coded squelch keyed onto the PCM of C transmit channels, the mirror of the DCS bank: the 23-bit
 * word of a code sent cyclically at 134.4 bit/s under the voice, the 134.4 Hz turn-off code behind it, both through one
 * shaping filter, added to the rows that hrfd_mod_* and hrfd_duc_transmit read.  PCM rows [C][n_blocks][512] int16 at 8 kS/s;
 * there is no n_pcm, and every sample of every block is written.  Exact integer arithmetic, the same on every device
 * (tests/dcsgen_model.py restates it); shifts are arithmetic.  Everything is per channel:
 *   sizes     C = 1..65536 channels, fixed at create; n_blocks = 1..HRFD_DCSGEN_MAX_BLOCKS = 1024; at most
 *             HRFD_DCSGEN_MAX_SEGMENTS = 8 segments per channel that have not ended; T = 1..HRFD_DCSGEN_MAX_TAPS = 512 taps,
 *             one list for the bank.
 *   time      the handle keeps one uint64 sample counter N, the stream time of the next call's first sample.  Every call
 *             advances it by 512 n_blocks, on the host.  Every stream time stays below 2^63.
 *   grid      u = n mod 28750, n the absolute stream time: 28750 = 23 x 1250 samples are exactly 483 = 21 x 23 bit times, so
 *             the pattern is periodic in u.  bit(n) = (word >> (floor(21 u / 1250) mod 23)) & 1: bit 0 of the word goes
 *             first.  The grid is absolute, not relative to a segment's start: a code queued again behind a cut goes on in
 *             phase.
 *   turn-off  sq(n) = +1 where floor(42 u / 1250) is even, else -1: a square wave of one bit time per period, 134.4 Hz.
 *   segment   {gap, length, tail, word, amp}, five uint32, with a start S (uint64 stream time).  word <= 0x7FFFFF: any 23
 *             bits (hrfd_dcs_code_word makes the one of a code); amp = 0..32767; length L = 1..2^32-2 samples, or
 *             HRFD_DCSGEN_FOREVER = 0xFFFFFFFF: no end; tail Q = 0..2^32-2 samples of turn-off code behind the code part
 *             (HRFD_DCSGEN_DEFAULT_TAIL = 1440: 180 ms); E = S + L + Q.  The raw level:
 *               r[n] = amp (2 bit(n) - 1)   for S <= n < S + L
 *               r[n] = amp sq(n)            for S + L <= n < E
 *               r[n] = 0                    where no segment of the channel covers n
 *             Segments of a channel never overlap; they may abut.
 *   shaping   acc[n] = sum_{j<T} h[j] r[n-j], h int16 in Q14 with sum |h| <= 65535, so acc is exact in int32 (65535 x 32767
 *             + 2^13 < 2^31); g[n] = (acc[n] + 2^13) >> 14, not saturated.  A new handle has the single tap 16384: g = r.
 *             There is no ramp of its own: the filter over the zeros outside a segment is the ramp.
 *   output    y = sat16(x + g); x is the input sample, or 0 when the call has no input (generate only).  clips[c] counts the
 *             samples where the saturation changed the value, until hrfd_dcsgen_reset.
 *   active    optional uint8 [C][n_blocks]: 1 where the block meets [S, E + T - 1) of any segment, so wherever g can be other
 *             than 0; else 0.  A caller keys a transmitter with it.
 *   queue     a segment has ended when E + 511 <= N, whatever T is: no later sample reaches it.  Segments that have ended
 *             leave the queue with the next call, hrfd_dcsgen_queue or hrfd_dcsgen_cut.
 * The output at stream time n is a pure function of n, the queue, the taps and x: however a stream is cut into calls, it comes
 * out the same.  With the single tap 16384 and no input, a code's samples are those of the host's restatement, api.dcs_levels.
 * Arguments are checked before any device is touched (HRFD_EINVAL without a GPU as well).  No setter waits for the device:
 * what changed is copied to the device on the next call's stream, ahead of its launch, and a call that already runs keeps the
 * queue and the taps it was launched with.  Calls may use different streams: each launch is ordered on the device behind the
 * handle's previous one.
 *   hrfd_dcsgen_set_taps       T taps, from the next call on; the queue and the clock stay (the filter keeps no state: r is a
 *                              function of the stream time)
 *   hrfd_dcsgen_queue          n = 1..8 segments on one channel, or on all (HRFD_ALL_CHANNELS).  The first begins at start +
 *                              segs[0].gap, each next one gap behind the end E of the one before.  start =
 *                              HRFD_DCSGEN_APPEND: max(N, the last E), per channel.  Refused whole (HRFD_EINVAL, nothing
 *                              queued on any channel): a start before N, an overlap, anything behind a FOREVER segment, a
 *                              ninth segment that has not ended, an amp above 32767, a length of 0, a word of 2^23 or more, a
 *                              tail of 2^32-1, a time at or above 2^63
 *   hrfd_dcsgen_cut            one channel, or all.  A segment in its code part at N (S <= N < S + L): the code part ends now,
 *                              L = N - S and E = N + (with_tail ? Q : 0) (kept below 2^63); dropped if S = N.  In its tail:
 *                              unchanged with with_tail, E = N without.  Not yet begun: dropped.  E <= N: untouched.  No
 *                              edit changes r before N
 *   hrfd_dcsgen_reset          empties every queue, N = 0, clips = 0; the taps stay
 *   hrfd_dcsgen_set_time       moves the clock only: the queues stay
 *   hrfd_dcsgen_time           N
 *   hrfd_dcsgen_pending        of one channel: the segments that have not ended at N, and the E of the last of them (N where
 *                              there is none, UINT64_MAX behind a FOREVER segment); either result may be NULL, not both
 *   hrfd_dcsgen_get_clips      clips[channel]; blocks until the handle's calls have run
 *   hrfd_dcsgen_process        host buffers, dense: pcm [C][n_blocks][512] or NULL (generate only) -> out [C][n_blocks][512],
 *                              active [C][n_blocks] or NULL.  out may be pcm itself; blocking
 *   hrfd_dcsgen_process_device device buffers; strides, in place, generate only and the overlap rule as
 *                              hrfd_tonegen_process_device: in place, a stretch of 2048 samples no segment reaches is neither
 *                              read nor written.  Asynchronous on `stream` (a hipStream_t, NULL = the handle's own)
 */
typedef struct hrfd_dcsgen hrfd_dcsgen;
typedef struct hrfd_dcsgen_segment
{
  uint32_t gap;                            /* samples of silence in front of the segment */
  uint32_t length;                         /* samples of the code, or HRFD_DCSGEN_FOREVER */
  uint32_t tail;                           /* samples of turn-off code behind them */
  uint32_t word;                           /* 23 bits, bit 0 first */
  uint32_t amp;
} hrfd_dcsgen_segment;
#define HRFD_DCSGEN_MAX_SEGMENTS 8
#define HRFD_DCSGEN_MAX_BLOCKS 1024
#define HRFD_DCSGEN_MAX_TAPS 512
#define HRFD_DCSGEN_FOREVER 0xffffffffu
#define HRFD_DCSGEN_DEFAULT_TAIL 1440u
#define HRFD_DCSGEN_APPEND UINT64_MAX
int hrfd_dcsgen_create(uint32_t n_channels, int device, hrfd_dcsgen **out);
int hrfd_dcsgen_destroy(hrfd_dcsgen *t);
int hrfd_dcsgen_set_taps(hrfd_dcsgen *t, const int16_t *taps, uint32_t n);
int hrfd_dcsgen_queue(hrfd_dcsgen *t, uint32_t channel, const hrfd_dcsgen_segment *segs, uint32_t n, uint64_t start);
int hrfd_dcsgen_cut(hrfd_dcsgen *t, uint32_t channel, int with_tail);
int hrfd_dcsgen_reset(hrfd_dcsgen *t);
int hrfd_dcsgen_set_time(hrfd_dcsgen *t, uint64_t N);
int hrfd_dcsgen_time(hrfd_dcsgen *t, uint64_t *N);
int hrfd_dcsgen_pending(hrfd_dcsgen *t, uint32_t channel, uint32_t *n_segments, uint64_t *end);
int hrfd_dcsgen_get_clips(hrfd_dcsgen *t, uint32_t channel, uint64_t *n);
int hrfd_dcsgen_process(hrfd_dcsgen *t, const int16_t *pcm, uint32_t n_blocks, int16_t *out, uint8_t *active);
int hrfd_dcsgen_process_device(hrfd_dcsgen *t, const int16_t *d_pcm, uint64_t channel_stride_bytes, uint32_t n_blocks,
                               int16_t *d_out, uint64_t out_stride_bytes, uint8_t *d_active, void *stream);

/* ------------------------------------------------------------------------------
 * AFSK bank: the PCM of C channels -> the packet data on them: audio frequency-shift keying, Bell 202 at 1200 baud (AX.25 /
 * APRS, MDC-1200) and Bell 103 at 300 baud among it.  A matched filter per tone and sample, a hard decision, and a bit clock
 * recovered from the decisions' transitions.  It reads what hrfd_rx_process_device / hrfd_ddc_receive write: PCM rows
 * [C][n_blocks][512] int16 at 8 kS/s and, optionally, n_pcm [C][n_blocks].  Exact integer arithmetic with a law of its own,
 * the same on every device and however a stream is cut into calls (tests/afsk_model.py restates it); shifts are arithmetic.
 * One modem for every channel of a handle; everything else is per channel:
 *   sizes     C = 1..65536 channels, fixed at create; n_blocks = 1..HRFD_AFSK_MAX_BLOCKS = 1024.
 *   modem     mark_step, space_step = round(f / 8000 * 2^32), the tone bank's, 1..2^31; baud_step = round(baud / 8000 * 2^32),
 *             1..2^31: at most one bit per sample; a window of W = 2..HRFD_AFSK_MAX_WINDOW = 32 samples; a loop shift
 *             A = 1..8; nrzi on or off.
 *   taps      for tone t in {mark, space} and k = 0..W-1: i = (((step_t k) mod 2^32 + 2^19) >> 20) & 4095,
 *             C_t[k] = clamp((COS[i] + 8) >> 4, -2047, 2047), S_t[k] the same from COS[(i - 1024) & 4095]  (COS: "DDC_COS").
 *   input     x[n] = the int16 sample, or 0 where n_pcm is given and the sample's position in its block is
 *             >= min(n_pcm[c][b], 512): the tone bank's law, time runs on.  Samples before the stream's start or a reset are 0.
 *   filter    I_t[n] = sum_k x[n-k] C_t[k], Q_t[n] the same with S_t.  |I| <= 32 x 32768 x 2047 < 2^31: every partial sum
 *             fits an int32.  P_t = I_t^2 + Q_t^2 < 2^63, in 64 bits; d[n] = P_mark - P_space (int64); h[n] = d[n] > 0.
 *   clock     a uint32 phase phi and the previous decision, both 0 at start.  For every sample, in this order:
 *               1. new = (phi + baud_step) mod 2^32
 *               2. if new < phi, a bit is sampled (below)
 *               3. if h[n] != h[n-1]: new -= ((int32)(new - 2^31)) >> A.  This pulls the transition towards mid-bit; it
 *                  never crosses 0 and never moves past 2^31
 *               4. phi = new
 *   bit       the sampled value is h[n]; with nrzi it is 1 - (h[n] ^ last), and then last = h[n] (last = 0 at start).  The
 *             output byte carries the value in bit 0 and the carrier flag in bit 1: P_mark[n] + P_space[n] > min_power
 *             (uint64, 0 unless set: digital silence carries no flag).
 *   outputs   bits: uint8, one row per channel; n_bits uint32 [C]: this call's count; bytes of a row from n_bits[c] on are
 *             not written.  A row holds at most hrfd_afsk_max_bits = ((512 n_blocks (baud_step + (2^31 >> A))) >> 32) + 1
 *             bits, because the phase advances by at most that much per sample.  hard (optional): uint8 [C][n_blocks][64],
 *             bit n & 7 of byte n >> 3 = h[n]: the discriminator's decisions, for a caller with a clock recovery of their own.
 *             bits and n_bits go together, both or neither; hard may be NULL, but not all three.  A call without bits does
 *             not run the clock: phi and last stay as they are, the samples and h[n-1] move on.
 *   state     per channel the last W - 1 samples, phi, h[n-1] and last: 18 dwords.
 *   defaults  1200 Hz mark, 2200 Hz space, 1200 baud, W = 8, A = 2, nrzi on; min_power 0.
 * Arguments are checked before any device is touched (HRFD_EINVAL without a GPU as well).  Setters never wait for the
 * device: what a setter changed goes to the device with the next call, ahead of its launch.  Calls may use different
 * streams: each launch is ordered on the device behind the handle's previous one (the state is the handle's), so a call
 * chains behind the receive call that filled its input when both are given the same stream.
 *   hrfd_afsk_set_modem        resets every channel: a history of another window length means nothing
 *   hrfd_afsk_set_carrier      min_power, for every channel; keeps the state
 *   hrfd_afsk_reset            the state of one channel, or of all (HRFD_ALL_CHANNELS), from the next call on
 *   hrfd_afsk_max_bits         the bound above for n_blocks under the handle's modem
 *   hrfd_afsk_process          host buffers, dense: pcm [C][n_blocks][512], n_pcm [C][n_blocks] or NULL -> bits
 *                              [C][hrfd_afsk_max_bits], n_bits [C], hard [C][n_blocks][64]; blocking
 *   hrfd_afsk_process_device   device buffers; input rows channel_stride_bytes apart (even and >= 1024 n_blocks), d_pcm at
 *                              any even address, d_n_pcm and d_n_bits 4-byte aligned; rows of d_bits bits_stride_bytes
 *                              apart, at least hrfd_afsk_max_bits (a smaller stride is refused); d_n_bits and d_hard dense.
 *                              Asynchronous on `stream` (a hipStream_t, NULL = the handle's own)
 */
typedef struct hrfd_afsk hrfd_afsk;
#define HRFD_AFSK_MAX_WINDOW 32
#define HRFD_AFSK_MAX_BLOCKS 1024
#define HRFD_AFSK_BIT 1u                   /* of a byte of bits: the value */
#define HRFD_AFSK_CARRIER 2u               /* of a byte of bits: the carrier flag */
int hrfd_afsk_create(uint32_t n_channels, int device, hrfd_afsk **out);
int hrfd_afsk_destroy(hrfd_afsk *a);
int hrfd_afsk_set_modem(hrfd_afsk *a, uint32_t mark_step, uint32_t space_step, uint32_t baud_step, uint32_t window,
                        uint32_t loop_shift, int nrzi);
int hrfd_afsk_set_carrier(hrfd_afsk *a, uint64_t min_power);
int hrfd_afsk_reset(hrfd_afsk *a, uint32_t channel);
int hrfd_afsk_max_bits(hrfd_afsk *a, uint32_t n_blocks, uint32_t *max_bits);
int hrfd_afsk_process(hrfd_afsk *a, const int16_t *pcm, const uint32_t *n_pcm, uint32_t n_blocks, uint8_t *bits, uint32_t *n_bits,
                      uint8_t *hard);
int hrfd_afsk_process_device(hrfd_afsk *a, const int16_t *d_pcm, uint64_t channel_stride_bytes, const uint32_t *d_n_pcm,
                             uint32_t n_blocks, uint8_t *d_bits, uint64_t bits_stride_bytes, uint32_t *d_n_bits, uint8_t *d_hard,
                             void *stream);

/* ------------------------------------------------------------------------------
 * AFSK generator bank: packet data keyed onto the PCM of C transmit channels: continuous-phase audio frequency-shift keying,
 * added to the rows that hrfd_mod_* and hrfd_duc_transmit read.  The mirror of the AFSK bank, which decodes what it sends,
 * on the tone generator's phase grid; the two generators compose by running one after the other, in place, on the same
 * rows.  PCM rows [C][n_blocks][512] int16 at 8 kS/s; there is no n_pcm, and every sample of every block is written.  Exact
 * integer arithmetic, the same on every device (tests/afskgen_model.py restates it); shifts are arithmetic.  Everything is
 * per channel, the modem included: it travels in the message.
 *   sizes     C = 1..65536 channels, fixed at create; n_blocks = 1..HRFD_AFSKGEN_MAX_BLOCKS = 1024; at most
 *             HRFD_AFSKGEN_MAX_MESSAGES = 4 messages per channel that have not ended.  The device's copy of the queues is
 *             4 KiB of levels and 128 bytes of descriptors a channel: 264 MiB at 65536 channels.
 *   time      the handle keeps one uint64 sample counter N, the stream time of the next call's first sample.  Every call
 *             advances it by 512 n_blocks, on the host.  Every stream time stays below 2^63.
 *   message   {gap, n_bits, mark_step, space_step, baud_step, amp, flags, pad}, eight uint32, with B = n_bits =
 *             1..HRFD_AFSKGEN_MAX_BITS = 8192 data bits d[i], one byte per bit of which only bit 0 counts (the format
 *             hrfd_afsk_process writes), and a start S (uint64 stream time).  The three steps = round(f / 8000 * 2^32),
 *             1..2^31; amp = 0..32767; flags: bit 0 = HRFD_AFSKGEN_NRZI, the others 0; pad = 0.
 *   levels    without NRZI l[i] = d[i] & 1.  With NRZI l[-1] = 1 (mark), l[i] = l[i-1] where d[i] & 1, else 1 - l[i-1]:
 *             the inverse of the AFSK bank's 1 - (h ^ last).
 *   length    L = ceil(B 2^32 / baud_step), the least k with (k baud_step) >> 32 >= B.  L >= 2^31 is refused.  E = S + L;
 *             E >= 2^63 is refused.
 *   law       at stream time n, k = n - S, 0 <= k < L:
 *               bit(k) = (k baud_step) >> 32              (a 64-bit product; < B by the definition of L)
 *               st(k) = l[bit(k)] ? mark_step : space_step
 *               theta(0) = 0, theta(k + 1) = (theta(k) + st(k)) mod 2^32       (the phase is continuous across the bits)
 *               i = ((theta(k) + 2^19) >> 20) & 4095
 *               s = COS[(i - 1024) & 4095]                (the tone generator's sine index: k = 0 is a zero crossing)
 *               v = (amp s + 2^14) >> 15
 *               e = min(k + 1, E - n, 64)
 *               g = (v e + 32) >> 6
 *             the tone generator's mix with one tone and its ramp of 64 samples (8 ms) at both ends.  With mark_step ==
 *             space_step a message is sample for sample the tone generator's segment of that start, length, step and amp.
 *   output    messages of one channel never overlap, so a sample has at most one g.  y = sat16(x + g); x is the input
 *             sample, or 0 when the call has no input (generate only).  clips[c] counts the samples where the saturation
 *             changed the value, until hrfd_afskgen_reset.
 *   active    optional uint8 [C][n_blocks]: 1 where a message has a sample in the block, else 0: the transmitter's key.
 * The output at stream time n is a pure function of n, the message and x: however a stream is cut into calls, it comes out
 * the same.  Messages that have ended (E <= N) leave the queue with the next call, hrfd_afskgen_queue or hrfd_afskgen_cut.
 * Arguments are checked before any device is touched (HRFD_EINVAL without a GPU as well).  No setter waits for the device:
 * what changed is copied to the device on the next call's stream, ahead of its launch, and a call that already runs keeps the
 * queue it was launched with.  Calls may use different streams: each launch is ordered on the device behind the handle's
 * previous one.
 *   hrfd_afskgen_queue          one message of bits[0..n_bits) on one channel, or on all (HRFD_ALL_CHANNELS).  It begins at
 *                               start + gap; start = HRFD_AFSKGEN_APPEND: max(N, the end of the channel's last message),
 *                               per channel.  Refused whole (HRFD_EINVAL, nothing queued on any channel): a start before
 *                               N, an overlap, a fifth message that has not ended, n_bits outside 1..8192, a step outside
 *                               1..2^31, an amp above 32767, other flags, a pad, L >= 2^31, a time at or above 2^63
 *   hrfd_afskgen_cut            one channel, or all: the message in progress at N (S <= N < E) is trimmed to end at
 *                               min(E, N + 64), which under the law is a ramp down; those not yet begun are dropped
 *   hrfd_afskgen_reset          empties every queue, N = 0, clips = 0
 *   hrfd_afskgen_set_time       moves the clock; refused while any channel holds a message that has not ended (a clock that
 *                               jumps into a message would need the sum of its steps up to there)
 *   hrfd_afskgen_time           N
 *   hrfd_afskgen_pending        of one channel: the messages that have not ended at N, and the end of the last of them (N
 *                               where there is none); either result may be NULL, not both
 *   hrfd_afskgen_get_clips      clips[channel]; blocks until the handle's calls have run
 *   hrfd_afskgen_process        host buffers, dense: pcm [C][n_blocks][512] or NULL (generate only) -> out [C][n_blocks][512],
 *                               active [C][n_blocks] or NULL.  out may be pcm itself; blocking
 *   hrfd_afskgen_process_device device buffers; input rows channel_stride_bytes apart, rows of d_out out_stride_bytes apart
 *                               (both even and >= 1024 n_blocks), d_pcm and d_out at any even address, d_active dense.  d_pcm
 *                               may be NULL (generate only; its stride is not looked at).  In place is allowed: d_out at exactly
 *                               the input's address with the same stride; a row no message touches in the call is then
 *                               neither read nor written.  Any other overlap of d_out and the input is refused.
 *                               Asynchronous on `stream` (a hipStream_t, NULL = the handle's own)
 */
typedef struct hrfd_afskgen hrfd_afskgen;
typedef struct hrfd_afskgen_message
{
  uint32_t gap;                            /* samples of silence in front of the message */
  uint32_t n_bits;                         /* data bits, 1..HRFD_AFSKGEN_MAX_BITS */
  uint32_t mark_step, space_step, baud_step;
  uint32_t amp;
  uint32_t flags;                          /* HRFD_AFSKGEN_NRZI or 0 */
  uint32_t pad;                            /* 0 */
} hrfd_afskgen_message;
#define HRFD_AFSKGEN_MAX_MESSAGES 4
#define HRFD_AFSKGEN_MAX_BITS 8192
#define HRFD_AFSKGEN_MAX_BLOCKS 1024
#define HRFD_AFSKGEN_NRZI 1u
#define HRFD_AFSKGEN_APPEND UINT64_MAX
int hrfd_afskgen_create(uint32_t n_channels, int device, hrfd_afskgen **out);
int hrfd_afskgen_destroy(hrfd_afskgen *g);
int hrfd_afskgen_queue(hrfd_afskgen *g, uint32_t channel, const hrfd_afskgen_message *msg, const uint8_t *bits, uint64_t start);
int hrfd_afskgen_cut(hrfd_afskgen *g, uint32_t channel);
int hrfd_afskgen_reset(hrfd_afskgen *g);
int hrfd_afskgen_set_time(hrfd_afskgen *g, uint64_t N);
int hrfd_afskgen_time(hrfd_afskgen *g, uint64_t *N);
int hrfd_afskgen_pending(hrfd_afskgen *g, uint32_t channel, uint32_t *n_messages, uint64_t *end);
int hrfd_afskgen_get_clips(hrfd_afskgen *g, uint32_t channel, uint64_t *n);
int hrfd_afskgen_process(hrfd_afskgen *g, const int16_t *pcm, uint32_t n_blocks, int16_t *out, uint8_t *active);
int hrfd_afskgen_process_device(hrfd_afskgen *g, const int16_t *d_pcm, uint64_t channel_stride_bytes, uint32_t n_blocks,
                                int16_t *d_out, uint64_t out_stride_bytes, uint8_t *d_active, void *stream);

/* ------------------------------------------------------------------------------
 * HDLC bank: the bits of C channels -> the packet frames in them (HDLC as AX.25 / APRS uses it): flags, bit stuffing, aborts
 * and the CRC-16/X.25 frame check, on the device.  It reads what hrfd_afsk_process_device writes, where it lies: rows of
 * bits, one byte a bit, bits_stride_bytes apart, and the counts d_n_bits [C], which the kernel reads on the device: no call
 * waits for it.  The law is per channel and bit by bit, the same on every device and however a stream is cut into calls
 * (tests/hdlc_model.py restates it):
 *   sizes     C = 1..65536 channels, fixed at create.  Per call max_bits = 1..HRFD_HDLC_MAX_BITS = 2^20; channel c uses
 *             min(d_n_bits[c], max_bits) bits.  bits_stride_bytes >= max_bits, rows at any address.  A longest payload of
 *             P = 1..HRFD_HDLC_MAX_PAYLOAD = 1021 bytes and a shortest of m = 1..P; a flag require_carrier.
 *   bit       a byte of the row: v = byte & HRFD_AFSK_BIT, c = (byte >> 1) & 1 (HRFD_AFSK_CARRIER).
 *   state     ones (0..7, saturating), in_frame, and the n bits collected so far, packed LSB first, at most
 *             cap = 8 (P + 2) + 7.  A channel starts with ones = 0, no frame open, n = 0.
 *   law       for every bit, in this order:
 *               0. if require_carrier and c == 0: in_frame = false.  The bit is then processed as usual
 *               1. v == 1: ones = min(7, ones + 1); if in_frame, append 1; if ones == 7, in_frame = false (an abort)
 *               2. v == 0 and ones == 6, a flag: if in_frame and n >= 7 + 8 (m + 2) and (n - 7) % 8 == 0, the first n - 7
 *                  bits are whole bytes, LSB first, the last two of them the check sequence, low byte first.  The frame is
 *                  good if the sequence is the CRC-16/X.25 of the bytes before it (equivalently: the CRC register, from
 *                  0xFFFF over all the bytes, ends at 0xF0B8), else it is bad.  Then in_frame = true, n = 0
 *               3. v == 0 and ones == 5: a stuffed zero, dropped
 *               4. v == 0 otherwise: if in_frame, append 0
 *               5. after any zero, ones = 0
 *             Appending when n == cap sets in_frame = false instead: an over-long frame is dead until the next flag.
 *             With require_carrier off the good frames are those of a plain flag / stuffing / CRC walk over the joined
 *             stream (api.hdlc_frames) that have at most P bytes.
 *   record    uint32 end_bit (the index in this call's row of the closing flag's last bit), uint16 n_payload, uint16 fcs
 *             (the check sequence as sent), the payload, zeros up to a multiple of 4: 8 + ((n_payload + 3) & ~3) bytes.
 *   outputs   a row of out_bytes bytes (a multiple of 4) per channel, rows out_stride_bytes apart: the good frames in stream
 *             order, one record behind the other.  A record that does not fit the row is dropped, and so is every good
 *             frame of the call behind it: d_n_frames [C] counts the records written, d_dropped [C] the good frames that were
 *             not (never partly written), d_n_bad [C] (optional) the bad frames of the call: a link-quality meter.  Bytes
 *             of a row behind its last record are not written.
 *   bound     a row of hrfd_hdlc_max_out(max_bits) bytes never drops: the closing bits of two frames of valid length lie at
 *             least 8 (m + 3) bits apart, so a call closes at most F = 1 + (max_bits - 1) / (8 (m + 3)); their payloads sum
 *             to at most min(F P, P + max_bits / 8) bytes (the carried partial frame and the call's bits); a record is at
 *             most 11 bytes more than its payload: 11 F + min(F P, P + max_bits / 8), rounded up to 4.
 *   state     per channel ones, in_frame, n and the partial frame: 260 dwords, on the device (twice: 2080 bytes a channel).
 *   defaults  m = 1, P = 512, require_carrier off.
 * Arguments are checked before any device is touched (HRFD_EINVAL without a GPU as well).  Setters never wait for the
 * device.  Calls may use different streams: each launch is ordered on the device behind the handle's previous one, so a call
 * chains behind the hrfd_afsk_process_device call that filled its input when both are given the same stream.
 *   hrfd_hdlc_set_limits          m and P; resets every channel: a partial frame under another bound means nothing
 *   hrfd_hdlc_set_require_carrier for every channel; keeps the state
 *   hrfd_hdlc_reset               the state of one channel, or of all (HRFD_ALL_CHANNELS), from the next call on
 *   hrfd_hdlc_max_out             the bound above for max_bits under the handle's limits
 *   hrfd_hdlc_process             host buffers, dense: bits [C][max_bits], n_bits [C] -> out [C][out_bytes], n_frames [C],
 *                                 n_bad [C] or NULL, dropped [C]; blocking
 *   hrfd_hdlc_process_device      device buffers; d_out 4-byte aligned, out_stride_bytes a multiple of 4 and >= out_bytes;
 *                                 the counts dense and 4-byte aligned.  Asynchronous on `stream` (a hipStream_t, NULL = the
 *                                 handle's own)
 */
typedef struct hrfd_hdlc hrfd_hdlc;
#define HRFD_HDLC_MAX_BITS (1u << 20)
#define HRFD_HDLC_MAX_PAYLOAD 1021
typedef struct hrfd_hdlc_record
{
  uint32_t end_bit;
  uint16_t n_payload;
  uint16_t fcs;
  /* the payload, zero-padded to a multiple of 4 */
} hrfd_hdlc_record;
int hrfd_hdlc_create(uint32_t n_channels, int device, hrfd_hdlc **out);
int hrfd_hdlc_destroy(hrfd_hdlc *h);
int hrfd_hdlc_set_limits(hrfd_hdlc *h, uint32_t min_payload, uint32_t max_payload);
int hrfd_hdlc_set_require_carrier(hrfd_hdlc *h, int on);
int hrfd_hdlc_reset(hrfd_hdlc *h, uint32_t channel);
int hrfd_hdlc_max_out(hrfd_hdlc *h, uint32_t max_bits, uint32_t *out_bytes);
int hrfd_hdlc_process(hrfd_hdlc *h, const uint8_t *bits, const uint32_t *n_bits, uint32_t max_bits, uint8_t *out, uint32_t out_bytes,
                      uint32_t *n_frames, uint32_t *n_bad, uint32_t *dropped);
int hrfd_hdlc_process_device(hrfd_hdlc *h, const uint8_t *d_bits, uint64_t bits_stride_bytes, const uint32_t *d_n_bits,
                             uint32_t max_bits, uint8_t *d_out, uint64_t out_stride_bytes, uint32_t out_bytes, uint32_t *d_n_frames,
                             uint32_t *d_n_bad, uint32_t *d_dropped, void *stream);

/* ------------------------------------------------------------------------------
 * HDLC framer bank: the packet frames of C channels -> the bits that say them, on the device: flags, the CRC-16/X.25 frame
 * check and bit stuffing.  The mirror of the HDLC bank: it reads rows of that bank's records where they lie and writes rows of
 * bits in the format hrfd_afskgen_queue takes and hrfd_hdlc_* reads.  The law is per channel, the same on every device
 * (tests/hdlcgen_model.py restates it):
 *   sizes     C = 1..65536 channels, fixed at create.  Per call in_bytes, a multiple of 4 (at least 4), and max_bits =
 *             1..HRFD_HDLCGEN_MAX_BITS = 2^20.  Three flag counts in the handle: lead 0..255, between 1..255, tail 1..255.
 *   input     per channel a row of in_bytes bytes of hrfd_hdlc_record: uint32 end_bit, uint16 n_payload, uint16 fcs, the
 *             payload, zeros up to a multiple of 4.  end_bit and fcs are ignored: the check sequence is always computed anew,
 *             so a row hrfd_hdlc_process_device wrote, with its d_n_frames, is framed again where it lies.  Rows are
 *             in_stride_bytes apart (a multiple of 4, >= in_bytes) and 4-byte aligned.  d_n_frames [C] says how many records
 *             a row holds; it is read on the device: no call waits for it.
 *   row       one byte per bit, 0 or 1: `lead` flags 0x7E; per frame the payload and its CRC-16/X.25 (reflected 0x1021 from
 *             0xFFFF, inverted), low byte first, every byte LSB first, with a zero inserted behind every fifth consecutive
 *             one: the count of ones starts at 0 at the frame's first bit and runs through the check sequence, and a fifth
 *             one that is the frame's last bit is followed by a zero as well; `between` flags between two frames, `tail`
 *             flags behind the last.  For the same flag counts this is api.hdlc_encode, bit for bit.  A channel that sends
 *             no frame writes nothing and has n_bits = 0.
 *   fit       frames are taken in row order.  The walk of a row ends at the first record that is malformed (its header or
 *             payload runs past in_bytes, or n_payload is outside 1..HRFD_HDLC_MAX_PAYLOAD) and at the first frame whose
 *             bits, with the flags in front of it and the tail flags still to come, would pass max_bits.  That frame and
 *             every one behind it are not sent: d_dropped [C] = d_n_frames - d_n_sent; d_n_sent [C] counts the frames
 *             framed, d_n_bits [C] is the row's length.  Bytes of a row behind n_bits are not written.
 *   bound     D = 8 (payload_bytes + 2 n_frames) data bits take at most D + floor(D / 5) bits (a frame of D_i data bits
 *             takes at most D_i + floor(D_i / 5), and the floors' sum is at most the sum's floor); with the
 *             lead + (n_frames - 1) between + tail flags that is a max_bits that never drops.
 *   defaults  lead 12, between 2, tail 3 (api.hdlc_encode's).
 * The bank carries nothing from call to call: a call's output is a complete message.  Arguments are checked before any
 * device is touched (HRFD_EINVAL without a GPU as well).  Setters never wait for the device: the flag counts travel with the
 * next launch.  Calls may use different streams: each launch is ordered on the device behind the handle's previous one, so
 * a call chains behind the hrfd_hdlc_process_device call, or the copy, that filled its input when both are given the same
 * stream.
 *   hrfd_hdlcgen_set_flags        the three flag counts, from the next call on
 *   hrfd_hdlcgen_max_bits         the bound above for n_frames frames (at least 1) of payload_bytes together under the
 *                                 handle's flag counts; refused if it passes 2^20
 *   hrfd_hdlcgen_process          host buffers, dense: records [C][in_bytes], n_frames [C] -> bits [C][max_bits], n_bits [C],
 *                                 n_sent [C] or NULL, dropped [C] or NULL; blocking
 *   hrfd_hdlcgen_process_device   device buffers; d_bits at any address, bits_stride_bytes >= max_bits; the counts dense
 *                                 and 4-byte aligned; d_n_sent and d_dropped may be NULL.  A row of bits may not overlap
 *                                 the records.  Asynchronous on `stream` (a hipStream_t, NULL = the handle's own)
 *   hrfd_hdlc_encode              one row under the same law on the host, bit by bit: no handle, no device.  records
 *                                 4-byte aligned, n_sent and dropped may be NULL; bits may not overlap the records
 */
typedef struct hrfd_hdlcgen hrfd_hdlcgen;
#define HRFD_HDLCGEN_MAX_BITS (1u << 20)
#define HRFD_HDLCGEN_MAX_FLAGS 255
int hrfd_hdlcgen_create(uint32_t n_channels, int device, hrfd_hdlcgen **out);
int hrfd_hdlcgen_destroy(hrfd_hdlcgen *h);
int hrfd_hdlcgen_set_flags(hrfd_hdlcgen *h, uint32_t n_lead_flags, uint32_t n_between, uint32_t n_tail_flags);
int hrfd_hdlcgen_max_bits(hrfd_hdlcgen *h, uint32_t n_frames, uint64_t payload_bytes, uint32_t *max_bits);
int hrfd_hdlcgen_process(hrfd_hdlcgen *h, const uint8_t *records, uint32_t in_bytes, const uint32_t *n_frames, uint8_t *bits,
                         uint32_t max_bits, uint32_t *n_bits, uint32_t *n_sent, uint32_t *dropped);
int hrfd_hdlcgen_process_device(hrfd_hdlcgen *h, const uint8_t *d_in, uint64_t in_stride_bytes, uint32_t in_bytes,
                                const uint32_t *d_n_frames, uint8_t *d_bits, uint64_t bits_stride_bytes, uint32_t max_bits,
                                uint32_t *d_n_bits, uint32_t *d_n_sent, uint32_t *d_dropped, void *stream);
int hrfd_hdlc_encode(const uint8_t *records, uint32_t in_bytes, uint32_t n_frames, uint32_t lead, uint32_t between, uint32_t tail,
                     uint8_t *bits, uint32_t max_bits, uint32_t *n_bits, uint32_t *n_sent, uint32_t *dropped);

/* ------------------------------------------------------------------------------
 * Introspection used by the tests: copy out the constant tables the kernels use.
 * name: "HB1","HB2","HB3","WBFM_D1","POST_D12","AUDIO_D40","FM_TUNER_D32","AM_D1",
 * "AM_D2","AM_D3","SSB_DELAY","SSB_HILBERT","INTERP_HB8","INTERP_HB3","INTERP_HB2",
 * "INTERP_HB1","INTERPSIG_S1", and the DDC bank's "DDC_COS" (4096 entries), "DDC_A2","DDC_A4","DDC_A8","DDC_B" (Q15 taps),
 * and the DUC bank's "DUC_A2","DUC_A4","DUC_A8" (Q15 taps), and the spectrum bank's "SPEC_HANN_<L>" (N entries),
 * "SPEC_COS_<L>", "SPEC_SIN_<L>" (N / 2 entries), L = 8..13, built on the host.
 * Copies min(cap, count) entries (out may be NULL to ask for the count) and returns the count, 0 if unknown. */
int hrfd_q15_table(const char *name, int16_t *out, int cap);
/* host-built atan2 table [256][256] (float bits) and dBFS table [257] */
int hrfd_atan2_table(float *out);
int hrfd_dbfs_table(int32_t *out);

#ifdef __cplusplus
}
#endif

#endif /* HRFD_H */
