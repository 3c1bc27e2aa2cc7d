"""QuartzNetCTC: the fused wav -> transcript fast path (one C-ABI call per batch).

This is what bench.py times and what ``VietASR.transcribe_batch`` uses.  It exists *in addition
to* the per-module NeuralModule classes in asr.py (same kernels, port tensors materialised);
both sit on libvasr_hip.so.  PyTorch is used for device memory and streams only.
"""
import threading

import numpy as np
import torch

from . import _lib, geometry
from .audio import pcm16_to_float, trim_silence as trim_audio
from .frontend_tables import frontend_description
from .stages import upload_masks


def _stream_ptr():
    return torch.cuda.current_stream().cuda_stream


def _require_gpu():
    if not torch.cuda.is_available():
        raise _lib.VasrError("viet-asr_amd needs a HIP device (torch.cuda.is_available() is False); "
                             "there is no CPU fallback for this path")


def compute_new_kernel_size(kernel_size, kernel_width):
    """JasperBlock's kernel_size_factor (parts/jasper.py:52-57): max(int(K * f), 1), plus one if that is even."""
    return geometry.odd_kernel(max(int(kernel_size * kernel_width), 1))


def blocks_from_config(jasper_cfg):
    """YAML block list (configs/*.yaml JasperEncoder.jasper) -> vasr_block_desc dicts.  ``kernel_size_factor`` is applied to
    the kernel here; groups and heads are read by groups_from_config."""
    def one(v):
        return int(v[0] if isinstance(v, (list, tuple)) else v)
    out = []
    for l in jasper_cfg:
        k = one(l["kernel"])
        f = float(l.get("kernel_size_factor", 1.0))
        if f != 1.0:
            k = compute_new_kernel_size(k, f)
        out.append(dict(filters=int(l["filters"]), repeat=int(l["repeat"]), kernel=k,
                        stride=one(l["stride"]), dilation=one(l["dilation"]),
                        residual=int(bool(l["residual"])), separable=int(bool(l.get("separable", False))),
                        residual_dense=int(bool(l.get("residual_dense", False)))))
    check_dense_layout(out)
    return out


def se_from_config(jasper_cfg):
    """Per block of a YAML block list: JasperBlock's SqueezeExcite reduction ratio (``se_reduction_ratio``, default 16,
    jasper.py:168-169), 0 for a block without ``se`` -- the argument of vasr_set_block_se."""
    out = []
    for l in jasper_cfg:
        if not l.get("se", False):
            out.append(0)
            continue
        r = l.get("se_reduction_ratio", 16)
        if int(r) != r or r <= 0:
            raise ValueError(f"se_reduction_ratio must be a positive integer, got {r!r}")
        if int(l["filters"]) // int(r) == 0:
            raise ValueError(f"se_reduction_ratio {r} leaves no hidden unit of {l['filters']} channels "
                             "(the reference builds a zero-width Linear)")
        out.append(int(r))
    return out


def groups_from_config(jasper_cfg):
    """Per block of a YAML block list: (groups, heads) -- JasperBlock's grouped main-branch convs followed by a channel shuffle
    (default 1) and the depthwise weights shared by ``heads`` rows (default -1: none), the arguments of vasr_set_block_groups.
    heads is -1 for a block that is not separable: the reference hands heads to the depthwise conv of a separable block only
    (parts/jasper.py:353-386) and ignores it elsewhere."""
    out = []
    for l in jasper_cfg:
        g, h = l.get("groups", 1), l.get("heads", -1)
        if int(g) != g or g < 1:
            raise ValueError(f"groups must be a positive integer, got {g!r}")
        if int(h) != h or (h != -1 and h < 1):
            raise ValueError(f"heads must be -1 or a positive integer, got {h!r}")
        out.append((int(g), int(h) if l.get("separable", False) else -1))
    return out


NORM_MODES = ("batch", "group", "instance", "layer")


ACTIVATIONS = {"relu": 0, "hardtanh": 1, "selu": 2}   # jasper_activations (parts/jasper.py:21-25) -> vasr_set_activation


def activation_from_config(enc_cfg):
    """JasperEncoder's ``activation`` and ``residual_mode`` (jasper.py:136-150, parts/jasper.py:438-441) -> the arguments of
    vasr_set_activation: (0 relu / 1 hardtanh / 2 selu, 0 add / 1 max).  An unknown activation raises KeyError, as the
    reference's dictionary lookup does; every residual_mode other than "add" combines the panes by max, as the reference's
    ``if self.residual_mode == "add": ... else: torch.max`` does."""
    act = ACTIVATIONS[enc_cfg.get("activation", "relu")]
    return act, 0 if enc_cfg.get("residual_mode", "add") == "add" else 1


def norm_from_config(enc_cfg, jasper_cfg):
    """Per block of a YAML block list: the GroupNorm group count of JasperEncoder's ``normalization_mode`` / ``norm_groups``
    (jasper.py:136-186, parts/jasper.py:342-391) -- 0 for "batch" (BatchNorm1d), ``norm_groups`` for "group" (-1, the
    default: the block's filters), the filters for "instance", 1 for "layer" -- the argument of vasr_set_block_norm.
    ValueError, as the reference raises: an unknown mode, or a group count that does not divide a block's filters."""
    mode = enc_cfg.get("normalization_mode", "batch")
    if mode not in NORM_MODES:
        raise ValueError(f"Normalization method ({mode}) does not match one of [batch, layer, group, instance].")
    if mode == "batch":
        return [0] * len(jasper_cfg)
    ng = enc_cfg.get("norm_groups", -1)
    if mode == "group" and (int(ng) != ng or (ng != -1 and ng < 1)):
        raise ValueError(f"norm_groups must be -1 or a positive integer, got {ng!r}")
    out = []
    for i, l in enumerate(jasper_cfg):
        c = int(l["filters"])
        g = {"instance": c, "layer": 1}.get(mode, c if ng == -1 else int(ng))
        if c % g:
            raise ValueError(f"block {i}: num_channels ({c}) must be divisible by num_groups ({g})")   # nn.GroupNorm
        out.append(g)
    return out


def check_dense_layout(blocks, feat_in=None):
    """Raise ValueError for the dense-residual layouts the reference builds but cannot run (JasperBlock.forward indexes
    xs[p] for every copied pane, parts/jasper.py:428-436, and only a dense block WITH residual hands xs + [out] on,
    :446-447): a dense block after a break in the run, after a dense block without residual, or a strided one.  A residual
    block that is not dense right after a dense run takes its residual from the run's input, xs[0] (:428-436): it must have
    that many input channels and no stride (``feat_in``: the encoder input width, for a run that starts at block 0)."""
    xs, seen, origin_c = 1, 0, feat_in
    for i, b in enumerate(blocks):
        cin = blocks[i - 1]["filters"] if i else feat_in
        width_differs = origin_c is not None and cin is not None and origin_c != cin     # (None: encoder input width unknown)
        if not b.get("residual_dense") and b["residual"] and xs > 1 and (b["stride"] > 1 or width_differs):
            raise ValueError(f"block {i}: a residual block after a dense run takes its residual from the run's input "
                             f"({origin_c} channels, block input {cin}, stride {b['stride']}) -- the reference fails here")
        if b.get("residual_dense"):
            seen += 1
            if b["residual"] and seen > xs:
                raise ValueError(f"block {i}: residual_dense block number {seen} would sum {seen} panes but only {xs} reach it -- "
                                 "dense blocks must form one contiguous run of residual blocks (the reference fails here)")
            if b["residual"] and b["stride"] > 1:
                raise ValueError(f"block {i}: a strided block cannot take a dense residual (its panes have other lengths)")
        if b.get("residual_dense") and b["residual"]:
            xs += 1
        else:
            xs, origin_c = 1, b["filters"]


def _pcm_to_float(s):
    """Integer PCM -> float32 scaled by 2^-(bits - 1) (AudioSegment._convert_samples_to_float32, parts/segment.py:61-74; exact for
    int16); anything else unchanged."""
    dt = getattr(s, "dtype", None)
    if dt is not None and dt.kind == "i":
        return s.astype(np.float32) * np.float32(1.0 / 2 ** (8 * dt.itemsize - 1))
    return s


def check_lengths(lens, n_fft, row_independent):
    """What every batch of signals is refused for, from its lengths: an empty batch, an empty signal and, with
    row_independent, a signal of n_fft / 2 samples or fewer (torch.stft cannot reflect it).  All ValueError."""
    if len(lens) == 0:
        raise ValueError("empty batch")
    if min(lens) == 0:
        raise ValueError("empty signal in batch")
    if row_independent and min(lens) <= n_fft // 2:
        raise ValueError(f"row-independent batching needs more than n_fft/2 = {n_fft // 2} samples "
                         f"per signal (got {min(lens)}): an unbatched call refuses such input too")


def all_int16(signals):
    return all(getattr(s, "dtype", None) == np.int16 for s in signals)


def collate(signals, n_fft=None, row_independent=False, keep_int16=False, out=None):
    """List of 1-D signals (float, or integer PCM) -> (batch [B, L] on the host, rows zero padded to the longest as
    ``seq_collate_fn`` pads them (parts/dataset.py:14-53); the lengths, a list).  L is at least 1.

    n_fft: the front end's; given, the lengths go through ``check_lengths`` first.  The batch is float32 and integer PCM
    rows are scaled as ``_pcm_to_float`` scales them -- also in a MIXED batch (the serving queue merges whatever arrives):
    assigned raw they would sit 2^15 too loud next to the float rows (found by tests/devtools/stress_serving.py, round 6).
    keep_int16: a batch in which EVERY row is int16 stays int16, to cross to the device at half the bytes.
    out: a [B, L] array to fill instead of a new one (pinned staging); its dtype decides, stale contents are overwritten."""
    lens = [len(s) for s in signals]
    if n_fft is not None:
        check_lengths(lens, n_fft, row_independent)
    if out is None:
        pcm16 = keep_int16 and all_int16(signals)
        out = np.zeros((len(signals), max(max(lens), 1)), dtype=np.int16 if pcm16 else np.float32)
    else:
        pcm16 = out.dtype == np.int16
    for i, s in enumerate(signals):
        out[i, : lens[i]] = s if pcm16 else _pcm_to_float(s)
        out[i, lens[i]:] = 0
    return out, lens


def handle_arguments(enc_cfg, feat_in):
    """A JasperEncoder section (``jasper``, ``activation``, ``normalization_mode``, ...) -> the encoder's keyword arguments of
    ``_lib.Handle``: feat_in, blocks, se, groups, norm, activation, residual_mode.  The block list is parsed here, once.
    NotImplementedError for what the library does not run: conv_mask=False, and a max residual beside any GroupNorm block."""
    jas = enc_cfg["jasper"]
    act, res_mode = activation_from_config(enc_cfg)
    if not enc_cfg.get("conv_mask", True):
        raise NotImplementedError("only conv_mask=True is implemented")
    norm = norm_from_config(enc_cfg, jas)
    if res_mode and any(norm):
        raise NotImplementedError("residual_mode='max' with group, instance or layer normalization is not implemented")
    return dict(feat_in=feat_in, blocks=blocks_from_config(jas), se=se_from_config(jas), groups=groups_from_config(jas),
                norm=norm, activation=act, residual_mode=res_mode)


class _Engine:
    """What the two engines share: a handle finalized from its states, a workspace that only grows, and the handle's
    row-independent switch set only when it changes."""

    def _finalize(self, handle, states, gemm):
        self.handle = handle
        for sd in states:
            handle.load_state_dict(sd)
        handle.finalize()
        if gemm is not None:
            handle.set_gemm_mode(gemm)
        self._ws = None
        self._row_independent = False

    def _grow(self, need):
        if self._ws is None or self._ws.numel() < need:
            self._ws = None
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._ws

    def _set_row_independent(self, on):
        self.handle.set_row_independent(on)
        self._row_independent = bool(on)


class QuartzNetCTC(_Engine):
    def __init__(self, model_definition, encoder_state, decoder_state, device="cuda:0", gemm=None):
        """gemm: None (library default: "f16x2"), "f16x2", "bf16x3", "fp32" or the reduced-precision opt-in "bf16x2" --
        see vasr_set_gemm_mode in include/vasr.h."""
        _require_gpu()
        self.device = torch.device(device)
        self.labels = list(model_definition["labels"])
        pre = dict(model_definition["AudioToMelSpectrogramPreprocessor"])
        enc = handle_arguments(model_definition["JasperEncoder"], pre.get("features", 64))
        self._blocks, self._se, self._norm = enc["blocks"], enc["se"], enc["norm"]
        self.frontend = frontend_description(pre)
        self.hop = self.frontend["hop_length"]
        with torch.cuda.device(self.device):
            self._finalize(_lib.Handle(frontend=self.frontend, dec_feat_in=self._blocks[-1]["filters"],
                                       num_classes=len(self.labels) + 1, **enc), (encoder_state, decoder_state), gemm)
        self._slots, self._copy_stream, self._launched = None, None, 0
        self._beam_stream = None
        self._beam_inflight = None                         # (done event, workgroups) of the last overlapped search

    # -- shapes
    def frames(self, samples):
        t = self.handle.mel_frames(samples)
        return t, self.handle.encoded_frames(t)

    def frame_seconds(self):
        """Seconds of audio per encoded frame: the front end's hop times the encoder's stride product -- what ``frames``
        divides by -- over the model's sample rate."""
        return self.hop * geometry.stride_product(self._blocks) / float(self.frontend["sample_rate"])

    def _workspace(self, batch, samples):
        return self._grow(self.handle.workspace_bytes(batch, samples=samples))

    def frames_of(self, length):
        """``frames(n)[1]`` for a [B] int64 tensor of sample counts, on its device: the encoded frames of each row alone -- the
        conv chain of vasr_encoded_frames in integer tensor ops, for lengths that exist on the device only (trim_silence)."""
        return geometry.frames_of(self._blocks, self.hop, length)

    def forward(self, wav, length, want_logp=False, want_pred=True, row_independent=False, trim_silence=False,
                _trim_buffers=None, augmentor=None, _lengths_host=None, spec_augment=None):
        """wav [B, L] f32 cuda (rows zero padded) -- or int16 PCM as it sits in a wav file: the front end scales it by 2^-15 as
        it reads it (vasr_transcribe_greedy_pcm16; the same bits as converting first) --, length [B] i64 cuda.

        Returns dict(ids [B,T'] i32, id_len [B] i32, pred [B,T'] i64, enc_len [B] f32, logp or None).
        Everything is enqueued on the current stream; nothing synchronises.

        row_independent=False is the reference's batched semantics (a row's result depends on the padded batch: reflect
        padding at the padded end, padded frames decoded).  True makes ids / id_len of every row what a batch-1 call on
        that row alone returns, bit for bit (vasr_set_row_independent in include/vasr.h); every length must then
        exceed n_fft / 2, which the caller checks (the lengths live on the device here).

        trim_silence=True cuts every row's leading and trailing silence on the device first, as ``AudioSegment(trim=True)``
        does in front of the reference's front end (segment.py:24-28; ``audio.trim_silence``, int16 stays int16): three more
        launches and no synchronisation -- the padded width stays L, so every frame count taken from L stays an upper
        bound.  The dict then also carries "trim_start" [B] i64 (the first kept sample of each row) and "length" [B] i64 (the
        trimmed lengths); ``frames_of(length)`` are the rows' own encoded frames.  With librosa's defaults a trimmed row keeps
        at least 512 samples of a longer one, so the n_fft / 2 rule checked on the untrimmed lengths still holds.

        augmentor: a ``perturb.AudioAugmentor`` (None: nothing changes).  The batch is perturbed on the device after the trim and in
        front of the front end, the reference's order in ``WaveformFeaturizer.process``; int16 PCM is scaled to float32 first.
        The parameters are drawn on the host from the rows' lengths (with trim_silence they are read back from the device: one
        synchronisation).  An impulse response makes the batch wider: every frame count then follows the new width, and the dict
        carries "length" [B] i64, the perturbed lengths.

        spec_augment: an ``asr.SpectrogramAugmentation`` (None: nothing changes -- the same launches, the same bits).  Its
        rectangles are drawn on the host for the [B, n_mels, T] feature tensor of this call, T from the final padded width (after
        the trim and ``augmentor``), uploaded without synchronising and zeroed in place between the front end's normalisation
        and the encoder (vasr_set_feature_masks: one more launch, no more memory), which is where the reference's DAG puts the
        module.  With row_independent=True row b is drawn as a batch-1 call on it alone would draw it -- over its own
        ``1 + length[b] // hop`` frames, cutout then augment, row after row -- so that its transcript equals that call's with the
        generator in the same state.  That needs the lengths on the host: where they exist only on the device (trim_silence, an
        ``augmentor``, or a direct call of this method) it costs one read-back, the synchronisation ``augmentor`` already costs.
        """
        if wav.device.type != "cuda" or wav.dtype not in (torch.float32, torch.int16) or not wav.is_contiguous():
            raise ValueError("wav must be a contiguous float32 (or int16 PCM) cuda tensor")
        if length.dtype != torch.int64 or length.device != wav.device:
            raise ValueError("length must be an int64 tensor on the same device")
        trim_start = None
        if trim_silence:
            out, start = _trim_buffers if _trim_buffers is not None else (None, None)
            wav, length, trim_start = trim_audio(wav, length, out=out, start=start)
        if augmentor is not None:
            if wav.dtype == torch.int16:
                wav = pcm16_to_float(wav)
            wav, length = augmentor.perturb_batch(wav, length, self.frontend["sample_rate"],
                                                  lengths_host=None if trim_silence else _lengths_host)
        B, L = wav.shape
        _, t1 = self.frames(L)
        ws = self._workspace(B, L)
        dev = wav.device
        ids = torch.empty((B, t1), dtype=torch.int32, device=dev)
        id_len = torch.empty((B,), dtype=torch.int32, device=dev)
        pred = torch.empty((B, t1), dtype=torch.int64, device=dev) if want_pred else None
        enc_len = torch.empty((B,), dtype=torch.float32, device=dev)
        logp = torch.empty((B, t1, len(self.labels) + 1), dtype=torch.float32, device=dev) if want_logp else None
        if bool(row_independent) != self._row_independent:
            self._set_row_independent(row_independent)
        masks = None
        if spec_augment is not None:
            row_frames = None
            if row_independent:
                on_host = _lengths_host is not None and not trim_silence and augmentor is None
                row_frames = [1 + int(n) // self.hop for n in (_lengths_host if on_host else length.cpu().tolist())]
            masks = upload_masks(*spec_augment.draw(B, self.frontend["n_mels"], self.frames(L)[0], row_frames), dev)
            self.handle.set_feature_masks(masks[0].data_ptr(), masks[1].data_ptr())
        entry = _lib.lib().vasr_transcribe_greedy_pcm16 if wav.dtype == torch.int16 else _lib.lib().vasr_transcribe_greedy_f32
        try:
            _lib.check(entry(
                self.handle.h, wav.data_ptr(), length.data_ptr(), B, L,
                pred.data_ptr() if pred is not None else None, ids.data_ptr(), id_len.data_ptr(),
                logp.data_ptr() if logp is not None else None, enc_len.data_ptr(),
                ws.data_ptr(), ws.numel(), _stream_ptr()))
        finally:
            if masks is not None:       # borrowed for this call only: the next one is unmasked again
                self.handle.set_feature_masks(None, None)
        r = dict(ids=ids, id_len=id_len, pred=pred, enc_len=enc_len, logp=logp)
        if trim_start is not None:
            r["trim_start"], r["length"] = trim_start, length
        if augmentor is not None:
            r["length"] = length
        return r

    def texts(self, ids, id_len):
        """Host side of helpers.py:32 -- ''.join(labels[c]) over the collapsed ids."""
        ids = ids.cpu().numpy()
        n = id_len.cpu().numpy()
        if (n < 0).any():      # vasr.h: id_len = -1 = the beam search's merge cells overflowed (cannot happen; reported, not hidden)
            raise _lib.VasrError("beam search reported an internal overflow (id_len = -1) for rows %s" % (n < 0).nonzero()[0].tolist())
        return ["".join(self.labels[c] for c in ids[b, : n[b]]) for b in range(ids.shape[0])]

    def transcribe(self, signals, row_independent=False, trim_silence=False, augmentor=None, spec_augment=None):
        """List of 1-D arrays (model sample rate; float, or int16 PCM) -> list of strings; zero-pad-to-max collate
        (parts/dataset.py:14-53).  row_independent, trim_silence, augmentor, spec_augment: see forward()."""
        return self.launch(signals, row_independent, trim_silence=trim_silence, augmentor=augmentor,
                           spec_augment=spec_augment).texts()

    def transcribe_beam(self, signals, beam_decoder, beam_width, row_independent=True, trim_silence=False, augmentor=None,
                        spec_augment=None):
        """Batched counterpart of the reference's beam wiring (infer.py:132-139, 159-160; batch 1 there): one forward
        pass for the log-probs, then viet_asr_amd.beam.BeamSearchDecoder over every row.  row_independent=True searches
        each row over its own frames (and reflects it at its own end): the transcripts of batch-1 calls.  trim_silence: see
        forward(); the rows' own frames then come from the trimmed lengths, on the device.  augmentor: see forward(); the
        rows' own frames come from the perturbed lengths.  spec_augment: see forward()."""
        r, own = self.forward_signals(signals, want_pred=False, row_independent=row_independent, trim_silence=trim_silence,
                                      augmentor=augmentor, spec_augment=spec_augment)
        # (without row_independent every frame of the padded batch is searched, as the reference searches its batch-1 tensor)
        return beam_decoder.decode_batch(r["logp"], beam_width, frames=own if row_independent else None)

    def forward_signals(self, signals, want_pred=True, row_independent=False, trim_silence=False, augmentor=None,
                        spec_augment=None):
        """List of 1-D signals at the model's rate (float, or integer PCM) -> (``forward(want_logp=True)``'s result dict of
        their zero-padded batch, the frames of every row: [B] int32 on the device).  With row_independent these are the row's
        own encoded frames, taken from the lengths where they last changed: on the device behind trim_silence or an
        ``augmentor`` (the dict's "length"), on the host otherwise.  Without, they are the encoder's lengths of the padded
        batch ("enc_len", truncated).  The other arguments: see forward()."""
        batch, lens = collate(signals, self.frontend["n_fft"], row_independent)
        r = self.forward(torch.from_numpy(batch).to(self.device), torch.tensor(lens, device=self.device),
                         want_logp=True, want_pred=want_pred, row_independent=row_independent, trim_silence=trim_silence,
                         augmentor=augmentor, _lengths_host=lens, spec_augment=spec_augment)
        if not row_independent:
            return r, r["enc_len"].to(torch.int32)
        if trim_silence or augmentor is not None:
            return r, self.frames_of(r["length"])
        return r, torch.tensor([self.frames(n)[1] for n in lens], dtype=torch.int32).to(self.device)

    def forward_beam(self, wav, length, beam_decoder, beam_width, frames=None, overlap=True):
        """Acoustic pass + beam search (+ LM) of one device-resident batch: the batched form of infer.py:146-160.

        overlap=True runs the search on a side stream: it occupies a compute unit per utterance up to 64 utterances (four
        wavefronts each, 1.3 ms at B = 64 x 501 frames, beam 128), a compute unit per four utterances beyond, so queued behind the
        log-probs of batch k it runs under the kernels of batch k + 1 instead of after them.  Returns dict(ids, id_len,
        score, done): ``done`` is an event on the side stream (None when overlap is off); wait for it -- or
        synchronise the device -- before reading the results from another stream."""
        # a search of the previous batch that is still queued or running holds a compute unit per four utterances while this
        # acoustic pass runs: the GEMM tile choice should fill whole rounds of what is left (vasr_set_busy_cus)
        busy = self._beam_inflight[1] if overlap and self._beam_inflight and not self._beam_inflight[0].query() else 0
        self.handle.set_busy_cus(busy)
        try:
            r = self.forward(wav, length, want_logp=True, want_pred=False)
        finally:
            self.handle.set_busy_cus(0)
        if not overlap:
            ids, n, score = beam_decoder.decode_ids(r["logp"], beam_width, frames)
            return dict(ids=ids, id_len=n, score=score, done=None, enc_len=r["enc_len"])
        if self._beam_stream is None:
            self._beam_stream = torch.cuda.Stream(self.device)
        main = torch.cuda.current_stream(self.device)
        ready = torch.cuda.Event()
        ready.record(main)
        with torch.cuda.stream(self._beam_stream):
            self._beam_stream.wait_event(ready)
            ids, n, score = beam_decoder.decode_ids(r["logp"], beam_width, frames)
            done = torch.cuda.Event()
            done.record(self._beam_stream)
        self._beam_inflight = (done, int(_lib.lib().vasr_beam_workgroups(int(r["logp"].shape[0]))))
        r["logp"].record_stream(self._beam_stream)     # allocated on the main stream, last read on the side stream
        return dict(ids=ids, id_len=n, score=score, done=done, enc_len=r["enc_len"])

    # -- long recordings in bounded memory
    def halo_mel_frames(self):
        """Half-width of the encoder's receptive field in mel frames (even): sum over the depthwise convolutions of
        (K - 1) / 2 * dilation, times the stride product in front of each."""
        return geometry.halo_mel_frames(self._blocks)

    def forward_long(self, wav, chunk_frames=4096, rows_per_pass=4, want_logp=False):
        """One long recording [L] (float32, on the device) in BOUNDED memory: the reference CLI skips files longer than
        10 s (infer.py:201-203); the one-call path handles any length but its workspace grows with it (2.6 GiB per hour of
        audio on QuartzNet12x1).  Here the log-mel features -- whose per-feature statistics span the whole recording
        (features.py:17-30), 256 bytes per frame -- are computed in one piece, and the encoder runs over windows of
        ``chunk_frames`` OUTPUT frames, each extended by the receptive-field halo on both sides (``halo_mel_frames``;
        zero padding only where the recording really ends), ``rows_per_pass`` windows at a time as the rows of one batch.
        Frames inside a window's halo are discarded, the kept ones see exactly the inputs of the one-pass computation:
        the same log-probs and predictions BIT FOR BIT in the fp32 and 3 x bf16 arithmetics; in the default 2 x fp16 one the operand
        scale follows the row a kernel works on (a window here, the recording there), the log-probs agree within the parity
        tolerance and a frame whose two best classes are closer than that may decode differently (round-6 campaign,
        tests/devtools/fuzz_long.py: 14 444 exact cases bit-equal; 2 such frames in 7 048 f16x2 recordings).  Returns dict(ids, id_len, pred, enc_len, logp or None, workspace_bytes)."""
        from . import stages
        if any(self._se):
            # the halo windows assume a finite receptive field; an SE's time mean makes it the whole recording
            raise NotImplementedError("forward_long: a model with squeeze-and-excitation (se) has no finite receptive field")
        if any(self._norm):
            # GroupNorm's statistics span each row's whole length, like an SE's time mean
            raise NotImplementedError("forward_long: a model with group, instance or layer normalization has no finite "
                                      "receptive field")
        if wav.dim() != 1 or wav.device.type != "cuda" or wav.dtype != torch.float32:
            raise ValueError("wav must be a 1-D float32 cuda tensor")
        h = self.handle
        L = wav.shape[0]
        mel, seq = stages.melspec(h, wav[None].contiguous(), torch.tensor([L], dtype=torch.int64, device=wav.device))
        T, seq0 = mel.shape[2], int(seq[0])
        T1 = h.encoded_frames(T)
        H, stride = self.halo_mel_frames(), geometry.stride_product(self._blocks)
        chunk_frames = max(int(chunk_frames), 1)
        jobs = []                                           # (mel lo, mel hi, mask length, first kept frame, kept frames)
        for o0 in range(0, T1, chunk_frames):
            o1 = min(o0 + chunk_frames, T1)
            lo = max(0, stride * o0 - H)
            lo -= lo % stride                                # windows start on the stride grid: same conv phase
            hi = min(T, stride * o1 + H)
            jobs.append((lo, hi, max(min(seq0, hi) - lo, 0), o0 - lo // stride, o1 - o0))
        c_out = self._blocks[-1]["filters"]
        V1 = len(self.labels) + 1
        logp = torch.empty((1, T1, V1), dtype=torch.float32, device=wav.device)
        ws_bytes, done = 0, 0
        for g in range(0, len(jobs), rows_per_pass):
            grp = jobs[g : g + rows_per_pass]
            W = max(hi - lo for lo, hi, *_ in grp)
            x = torch.zeros((len(grp), mel.shape[1], W), dtype=torch.float32, device=wav.device)
            for r, (lo, hi, *_rest) in enumerate(grp):
                x[r, :, : hi - lo] = mel[0, :, lo:hi]
            lens = torch.tensor([j[2] for j in grp], dtype=torch.int64, device=wav.device)
            enc, _ = stages.encoder(h, x, lens, c_out)
            ws_bytes = max(ws_bytes, h.workspace_bytes(len(grp), mel_frames=W))
            for r, (_lo, _hi, _ml, skip, keep) in enumerate(grp):
                piece = enc[r : r + 1, :, skip : skip + keep].contiguous()
                logp[:, done : done + keep] = stages.decoder(h, piece)
                done += keep
        pred = stages.greedy_argmax(logp)
        ids, id_len = stages.ctc_collapse(pred, V1 - 1)
        enc_len = torch.tensor([float(self._encoded_length(seq0))], dtype=torch.float32, device=wav.device)
        return dict(ids=ids, id_len=id_len, pred=pred, enc_len=enc_len, logp=logp if want_logp else None,
                    workspace_bytes=ws_bytes, one_pass_workspace_bytes=h.workspace_bytes(1, samples=L))

    def _encoded_length(self, seq):
        """MaskedConv1d.get_seq_len chain (jasper.py:108-111, quirk Q3) on the host: float result, truncated between convs."""
        return geometry.encoded_length(self._blocks, seq)

    # -- pipelined host path: pinned staging, copies on their own stream, two batches in flight
    def launch(self, signals, row_independent=False, after_forward=None, trim_silence=False, augmentor=None,
               spec_augment=None):
        """Enqueue one batch and return at once; ``.texts()`` of the returned PendingBatch waits for it.

        Two staging slots alternate: while batch k computes, batch k+1 is collated into pinned memory and its
        host->device copy runs on a separate stream (``torch.from_numpy(x).to(device)`` from pageable memory costs
        more than the whole forward pass of a 64 x 10 s batch).  int16 PCM signals cross PCIe as int16 and are scaled
        by 2^-15 on the device (segment.py:61-74) -- half the bytes, same floats.

        after_forward(out): called with ``forward``'s result dict on the compute stream, right after the forward pass is
        enqueued and before its results are copied out -- device-side consumers of the ids (``metrics.ErrorRate.update``)
        hook in here; it must not synchronise.

        trim_silence: see forward(); the slot keeps a second device buffer for the trimmed batch and one for the starts.
        augmentor: see forward(); the staging for the ids is sized by ``augmentor.max_augmentation_length``.
        spec_augment: see forward(); the rectangles are drawn here, on the host, while the previous batch computes.
        """
        check_lengths([len(s) for s in signals], self.frontend["n_fft"], row_independent)
        if self._slots is None:
            self._slots = [_Slot(self), _Slot(self)]
            self._copy_stream = torch.cuda.Stream(self.device)
        slot = self._slots[self._launched % 2]
        self._launched += 1
        return slot.launch(signals, row_independent, after_forward, trim_silence, augmentor, spec_augment)


class QuartzNetClassifier(_Engine):
    """The fused wav -> class fast path of the speech-command / keyword models (one C-ABI call per batch,
    vasr_classify_f32): AudioToMelSpectrogramPreprocessor -> CropOrPadSpectrogramAugmentation(audio_length) -> JasperEncoder ->
    JasperDecoderForClassification.  Lives beside QuartzNetCTC; the per-module classes in asr.py run the same kernels."""

    def __init__(self, model_definition, encoder_state, decoder_state, audio_length, labels=None, pooling_type="avg",
                 device="cuda:0", gemm=None):
        """decoder_state: JasperDecoderForClassification's state_dict (decoder_layers.0.weight [num_classes][feat_in], .bias);
        labels: class names for classify() (None: it returns indices); gemm: as QuartzNetCTC's."""
        _require_gpu()
        if pooling_type not in ("avg", "max"):
            raise ValueError('Pooling type chosen is not valid. Must be either `avg` or `max`')
        self.device = torch.device(device)
        self.audio_length = int(audio_length)
        if self.audio_length <= 0:
            raise ValueError(f"audio_length must be positive, got {audio_length!r}")
        self.labels = list(labels) if labels is not None else None
        pre = dict(model_definition["AudioToMelSpectrogramPreprocessor"])
        enc = handle_arguments(model_definition["JasperEncoder"], pre.get("features", 64))
        self.frontend = frontend_description(pre)
        w = np.asarray(decoder_state["decoder_layers.0.weight"].detach().cpu().numpy()
                       if hasattr(decoder_state["decoder_layers.0.weight"], "detach") else decoder_state["decoder_layers.0.weight"])
        self.num_classes = int(w.shape[0])
        if self.labels is not None and len(self.labels) != self.num_classes:
            raise ValueError(f"{len(self.labels)} labels for {self.num_classes} classes")
        with torch.cuda.device(self.device):
            head = (enc["blocks"][-1]["filters"], self.num_classes, 0 if pooling_type == "avg" else 1)
            self._finalize(_lib.Handle(frontend=self.frontend, classifier=head, **enc), (encoder_state, decoder_state), gemm)

    def forward(self, wav, length, offsets=None, softmax=False, row_independent=False, want_mel=False, trim_silence=False):
        """wav [B, L] f32 cuda (rows zero padded), length [B] i64 cuda -> logits [B, num_classes] f32, or probabilities
        (softmax=True: F.softmax(logits, -1)).  Enqueued on the current stream; nothing synchronises.

        offsets [B] i64: where each row is cut when the batch is wider than audio_length frames; None draws them as the
        reference does, torch.randint(0, T - audio_length + 1, [B]) on the default CPU generator (reproducible under
        torch.manual_seed); an explicit array makes the crop reproducible without the generator.  row_independent: as
        QuartzNetCTC.forward -- every row is reflected, cut (its offset clamped into its own width) or centred as a batch-1
        call on it alone would be, and its output is that call's, bit for bit; every length must then exceed n_fft / 2.
        want_mel: return (out, mel [B, n_mels, audio_length]), the encoder's input.  trim_silence: as QuartzNetCTC.forward --
        every row's leading and trailing silence is cut on the device in front of the front end, the padded width stays L."""
        if wav.device.type != "cuda" or wav.dtype != torch.float32 or not wav.is_contiguous():
            raise ValueError("wav must be a contiguous float32 cuda tensor")
        if length.dtype != torch.int64 or length.device != wav.device:
            raise ValueError("length must be an int64 tensor on the same device")
        if trim_silence:
            wav, length, _ = trim_audio(wav, length)
        B, L = wav.shape
        T = self.handle.mel_frames(L)
        if offsets is None and T > self.audio_length:
            offsets = torch.randint(low=0, high=T - self.audio_length + 1, size=[B])
        off = None
        if offsets is not None:
            off = torch.as_tensor(offsets).to(device=wav.device, dtype=torch.int64).contiguous()
            if off.shape != (B,):
                raise ValueError(f"offsets must have shape ({B},), got {tuple(off.shape)}")
        ws = self._grow(int(_lib.lib().vasr_classify_workspace_bytes(self.handle.h, B, L, self.audio_length)))
        if bool(row_independent) != self._row_independent:
            self._set_row_independent(row_independent)
        out = torch.empty((B, self.num_classes), dtype=torch.float32, device=wav.device)
        mel = torch.empty((B, self.frontend["n_mels"], self.audio_length), dtype=torch.float32, device=wav.device) if want_mel else None
        _lib.check(_lib.lib().vasr_classify_f32(
            self.handle.h, wav.data_ptr(), length.data_ptr(), B, L, self.audio_length, off.data_ptr() if off is not None else None,
            int(bool(softmax)), out.data_ptr(), mel.data_ptr() if mel is not None else None, ws.data_ptr(), ws.numel(),
            _stream_ptr()))
        return (out, mel) if want_mel else out

    def classify(self, signals, offsets=None, row_independent=False, trim_silence=False):
        """List of 1-D arrays (model sample rate; float, or integer PCM) -> the arg-max class index per signal, or its label
        where ``labels`` was given; zero-pad-to-max collate (parts/dataset.py:14-53).  Short inputs follow QuartzNetCTC's
        rules: no empty batch or signal, and more than n_fft / 2 samples per signal with row_independent.  trim_silence: see
        forward()."""
        out = self.forward(*self._collate(signals, row_independent), offsets=offsets, row_independent=row_independent,
                           trim_silence=trim_silence)
        idx = out.argmax(-1).cpu().tolist()
        return [self.labels[i] for i in idx] if self.labels is not None else idx

    def _collate(self, signals, row_independent):
        """classify's collate: (wav [B, L] f32, length [B] i64) on the device, rows zero padded to the longest."""
        batch, lens = collate(signals, self.frontend["n_fft"], row_independent)
        return torch.from_numpy(batch).to(self.device), torch.tensor(lens, device=self.device)

    def classify_topk(self, signals, k, offsets=None, row_independent=False, trim_silence=False):
        """``classify``'s input -> per signal the list of its k best (label or index, softmax probability) pairs, best first:
        larger logit first, the lower class index first among equal ones (``stages.classification_scores``).  The same
        collate and forward pass as ``classify``; one device-to-host copy at the end."""
        from . import stages
        k = int(k)
        if not 1 <= k <= min(16, self.num_classes):
            raise ValueError(f"k must be in 1..{min(16, self.num_classes)}, got {k}")
        out = self.forward(*self._collate(signals, row_independent), offsets=offsets, row_independent=row_independent,
                           trim_silence=trim_silence)
        top = stages.classification_scores(out, k=k, want_prob=True)
        # one copy: the indices (exact in float32, below 2^24) next to the probabilities
        both = torch.cat([top["indices"].to(torch.float32), top["probs"]], dim=1).cpu().tolist()
        name = (lambda i: self.labels[i]) if self.labels is not None else (lambda i: i)
        return [[(name(int(r[j])), r[k + j]) for j in range(k)] for r in both]

    def evaluate_manifest(self, manifest_filepath, batch_size=64, top_k=(1,), offsets=None, row_independent=False,
                          trim_silence=False):
        """Top-k accuracy and evaluation loss over a labelled manifest: -> (predictions, ``TopKAccuracy.compute()``), the
        dict {"accuracy": {k: float}, "correct": {k: int}, "samples": int, "eval_loss": float}; predictions: the top-1 class
        (label, or index without ``labels``) per kept manifest entry, in manifest order.
        Where the data layer shards the manifest over a process group, "entry" -- here and for ``offsets`` -- means THIS
        rank's entries, still in manifest order; a ``TopKAccuracy`` of your own with ``compute(reduce=True)`` gives the
        global figure.

        The manifest is walked by ``AudioToSpeechLabelDataLayer`` (its line format and duration filter; the ``labels`` given
        to this engine map the manifest's labels to classes, without them the manifest must hold class indices).  Each
        batch crosses from pinned memory, and its scoring (one vasr_class_scores_f32 launch: top-1, rank and loss) is
        enqueued right behind its forward pass; the only synchronisation before the final ``compute`` is the copy of the
        predictions after the last batch.  offsets: None (drawn per batch as ``forward`` draws them) or one crop offset per
        kept manifest entry, in manifest order.  trim_silence: see forward() -- the data layer hands out untrimmed host
        tensors (its own ``trim_silence`` is not implemented); the trim happens here, on the device, per batch."""
        from . import stages
        from .data_layer import AudioToSpeechLabelDataLayer
        from .metrics import TopKAccuracy
        labels = self.labels if self.labels is not None else list(range(self.num_classes))
        layer = AudioToSpeechLabelDataLayer(manifest_filepath, labels, batch_size, sample_rate=self.frontend["sample_rate"])
        order = layer.utterance_order()          # positions in the whole filtered manifest, of this rank's entries only
        slot = {g: p for p, g in enumerate(sorted(order))}
        if offsets is not None and len(offsets) != len(order):
            raise ValueError(f"{len(offsets)} offsets for {len(order)} manifest entries")
        metric = TopKAccuracy(top_k)
        picks, staged, pos = [], [], 0          # staged: pinned batches, alive until the copies that read them have run
        for audio, a_len, label, _ in layer.data_iterator:
            B = audio.shape[0]
            check_lengths(a_len.tolist(), self.frontend["n_fft"], row_independent)
            off = None
            if offsets is not None:
                off = torch.tensor([int(offsets[slot[i]]) for i in order[pos : pos + B]], dtype=torch.int64).pin_memory()
            pos += B
            host = [t.pin_memory() for t in (audio, a_len, label)] + ([off] if off is not None else [])
            dev = [t.to(self.device, non_blocking=True) for t in host]
            done = torch.cuda.Event()
            done.record(torch.cuda.current_stream(self.device))
            staged = [(e, h) for e, h in staged if not e.query()] + [(done, host)]
            out = self.forward(dev[0], dev[1], offsets=dev[3] if off is not None else None, row_independent=row_independent,
                               trim_silence=trim_silence)
            scores = stages.classification_scores(out, dev[2], k=1)
            metric.add_scores(scores["rank"], scores["loss"])
            picks.append(scores["indices"].view(-1))
        idx = torch.cat(picks).cpu().tolist() if picks else []
        predictions = [None] * len(order)
        for i, c in zip(order, idx):
            predictions[slot[i]] = self.labels[c] if self.labels is not None else c
        return predictions, metric.compute()


class PendingBatch:
    """Result handle of QuartzNetCTC.launch()."""

    def __init__(self, slot, batch, frames):
        self._slot, self._batch, self._frames = slot, batch, frames
        self._lock = threading.Lock()
        self._texts = None

    def done(self):
        return self._texts is not None or self._slot.ev_out.query()

    def texts(self):
        with self._lock:
            if self._texts is None:
                s, B, t1 = self._slot, self._batch, self._frames
                s.ev_out.synchronize()
                ids = s.pin_ids[: B * t1].view(B, t1).numpy()
                n = s.pin_idlen[:B].numpy()
                labels = s.eng.labels
                self._texts = ["".join(labels[c] for c in ids[b, : n[b]]) for b in range(B)]
                s.pending = None
            return self._texts


class _Slot:
    """Pinned staging + device input buffers of one in-flight batch (grown on demand, never shrunk)."""

    def __init__(self, eng):
        self.eng = eng
        self.pin = self.dev = None
        self.dev_trim = self.dev_start = None     # trim_silence: the trimmed batch and the rows' starts
        self.pin_len = self.dev_len = None
        self.pin_ids = self.pin_idlen = None
        self.out = None               # device outputs of the batch in flight (kept alive until its results are read)
        self.pending = None
        self.ev_h2d = torch.cuda.Event()
        self.ev_out = torch.cuda.Event()

    def _reserve_trim(self, B, nbytes):
        dev = self.eng.device
        if self.dev_trim is None or self.dev_trim.numel() < nbytes:
            self.dev_trim = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        if self.dev_start is None or self.dev_start.numel() < B:
            self.dev_start = torch.empty(B, dtype=torch.int64, device=dev)

    def _reserve(self, B, nbytes, t1, pcm16):
        dev = self.eng.device
        if self.pin is None or self.pin.numel() < nbytes:
            self.pin = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
            self.dev = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        if self.pin_len is None or self.pin_len.numel() < B:
            self.pin_len = torch.empty(B, dtype=torch.int64, pin_memory=True)
            self.dev_len = torch.empty(B, dtype=torch.int64, device=dev)
            self.pin_idlen = torch.empty(B, dtype=torch.int32, pin_memory=True)
        if self.pin_ids is None or self.pin_ids.numel() < B * t1:
            self.pin_ids = torch.empty(B * t1, dtype=torch.int32, pin_memory=True)

    def launch(self, signals, row_independent=False, after_forward=None, trim_silence=False, augmentor=None,
               spec_augment=None):
        eng = self.eng
        if self.pending is not None:
            self.pending.texts()          # the slot's previous batch: fetch before its buffers are overwritten
        B, L = len(signals), max(len(s) for s in signals)
        pcm16 = all_int16(signals)
        dtype, item = (torch.int16, 2) if pcm16 else (torch.float32, 4)
        nbytes = B * L * item
        _, t1 = eng.frames(L)
        if augmentor is not None:         # the widest the batch can become: the staging for the ids holds that many frames
            t1 = eng.frames(int(augmentor.max_augmentation_length(L, eng.frontend["sample_rate"])))[1]
        with torch.cuda.device(eng.device):
            self.ev_out.synchronize()     # batch k-2 has left the device buffers
            self._reserve(B, nbytes, t1, pcm16)
            trim_buffers = None
            if trim_silence:
                self._reserve_trim(B, nbytes)
                trim_buffers = (self.dev_trim[:nbytes].view(dtype).view(B, L), self.dev_start[:B])
            _, lens = collate(signals, out=self.pin[:nbytes].view(dtype).view(B, L).numpy())
            self.pin_len[:B] = torch.tensor(lens, dtype=torch.int64)
            comp = torch.cuda.current_stream(eng.device)
            with torch.cuda.stream(eng._copy_stream):
                self.dev[:nbytes].copy_(self.pin[:nbytes], non_blocking=True)
                self.dev_len[:B].copy_(self.pin_len[:B], non_blocking=True)
                self.ev_h2d.record(eng._copy_stream)
            comp.wait_event(self.ev_h2d)
            wav = self.dev[:nbytes].view(dtype).view(B, L)
            # (int16 PCM goes into the front end as it is: scaled by 2^-15 in the STFT kernel's staging load)
            self.out = eng.forward(wav, self.dev_len[:B], want_pred=False, row_independent=row_independent,
                                   trim_silence=trim_silence, _trim_buffers=trim_buffers, augmentor=augmentor,
                                   _lengths_host=lens, spec_augment=spec_augment)
            t1 = self.out["ids"].shape[1]  # the width the batch got (an impulse response widens it)
            if after_forward is not None:
                after_forward(self.out)
            self.pin_ids[: B * t1].copy_(self.out["ids"].view(-1), non_blocking=True)
            self.pin_idlen[:B].copy_(self.out["id_len"], non_blocking=True)
            self.ev_out.record(comp)
        self.pending = PendingBatch(self, B, t1)
        return self.pending
