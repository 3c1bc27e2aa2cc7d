"""HIP-backed counterparts of the reference's ASR NeuralModules (``nemo.collections.asr``).

Same class names, constructor signatures, port names / neural types and checkpoint
(``state_dict``) layout as the reference, so that infer.py-style code only changes its import:

    import viet_asr_amd.asr as nemo_asr

Every ``forward`` runs hand-written gfx950 kernels through libvasr_hip.so (stages.py); there is no
torch-eager or CPU fallback -- constructing modules and wiring the DAG works anywhere, running a
forward without a HIP device raises.
"""
import torch
import torch.nn as nn

from . import _lib, stages
from .core import (AcousticEncodedRepresentation, AudioSignal, DataLayerNM, DeviceType, LabelsType, LengthsType,
                   LogitsType, LogprobsType, LossType, MelSpectrogramType, NeuralType, NonTrainableNM, PredictionsType,
                   SpectrogramType, TrainableNM)
from .engine import check_dense_layout, collate, handle_arguments
from .frontend_tables import frontend_description
from .geometry import odd_kernel

__all__ = ["AudioToMelSpectrogramPreprocessor", "CropOrPadSpectrogramAugmentation", "JasperEncoder", "JasperDecoderForCTC",
           "JasperDecoderForClassification", "GreedyCTCDecoder", "BeamSearchDecoderWithLM", "AudioDataLayer", "CTCLossNM",
           "SpecAugment", "SpecCutout", "SpectrogramAugmentation", "MultiplyBatch"]


def _no_gpu():
    return _lib.VasrError("viet-asr_amd needs a HIP device (torch.cuda.is_available() is False); "
                          "there is no CPU fallback for this path")


class AudioToMelSpectrogramPreprocessor(NonTrainableNM):
    """nemo/collections/asr/audio_preprocessing.py:212-383 (forward :78-87 -> parts/features.py:245-301)."""

    @property
    def input_ports(self):
        return {"input_signal": NeuralType(("B", "T"), AudioSignal(freq=self._sample_rate)),
                "length": NeuralType(tuple("B"), LengthsType())}

    @property
    def output_ports(self):
        return {"processed_signal": NeuralType(("B", "D", "T"), MelSpectrogramType()),
                "processed_length": NeuralType(tuple("B"), LengthsType())}

    def __init__(self, sample_rate=16000, window_size=0.02, window_stride=0.01, n_window_size=None,
                 n_window_stride=None, window="hann", normalize="per_feature", n_fft=None, preemph=0.97,
                 features=64, lowfreq=0, highfreq=None, log=True, log_zero_guard_type="add",
                 log_zero_guard_value=2 ** -24, dither=1e-5, pad_to=16, frame_splicing=1, stft_conv=False,
                 pad_value=0, mag_power=2.0):
        self._sample_rate = sample_rate
        super().__init__()
        if log_zero_guard_type not in ("add", "clamp"):
            raise ValueError(f"{self} received {log_zero_guard_type} for the log_zero_guard_type parameter. "
                             "It must be either 'add' or 'clamp'.")
        self._desc = frontend_description(dict(
            sample_rate=sample_rate, window_size=window_size, window_stride=window_stride,
            n_window_size=n_window_size, n_window_stride=n_window_stride, window=window, normalize=normalize,
            n_fft=n_fft, preemph=preemph, features=features, lowfreq=lowfreq, highfreq=highfreq, log=log,
            log_zero_guard_type=log_zero_guard_type, log_zero_guard_value=log_zero_guard_value,
            frame_splicing=frame_splicing, stft_conv=stft_conv, pad_value=pad_value, mag_power=mag_power))
        # dither (features.py:250-251): `x += dither * torch.randn_like(x)` -- the SAME torch call on the same device tensor, in
        # place like the reference (SURVEY section 8b "ownership"), so that under one torch.manual_seed this module and the
        # reference's draw the same noise on the same device; infer.py:89 forces 0.  pad_to: FilterbankFeatures zero-pads T up
        # to a multiple of self.pad_to in training mode -- the mode the executor leaves this NonTrainableNM in, quirk Q1 -- and
        # of 16 in eval mode (features.py:292-300); infer.py:90 sets 0 = no padding.  A non-zero pad_to is applied here the way
        # the reference's (training-mode) branch does it: extra all-zero frames appended on the device.
        if dither is not None and dither < 0:
            raise ValueError(f"dither must be >= 0, got {dither!r}")
        if pad_to == "max":
            # features.py:209 evaluates `pad_to > 0` in the constructor: with the string the docstring advertises
            # (audio_preprocessing.py:261-262, features.py:295-296) the reference itself raises this TypeError
            raise TypeError("'>' not supported between instances of 'str' and 'int' (pad_to='max': the reference's own "
                            "constructor fails at parts/features.py:209)")
        if pad_to is not None and (int(pad_to) != pad_to or pad_to < 0):
            raise ValueError(f"pad_to must be a non-negative integer, got {pad_to!r}")
        self.dither, self.pad_to = float(dither or 0.0), int(pad_to or 0)
        self.win_length, self.hop_length = self._desc["win_length"], self._desc["hop_length"]
        self._handle = None

    def _get_handle(self):
        if self._handle is None:
            if not torch.cuda.is_available():
                raise _no_gpu()
            self._handle = _lib.Handle(frontend=self._desc)
            self._handle.finalize()
        return self._handle

    @property
    def filter_banks(self):
        return torch.from_numpy(self._desc["filterbank"]).unsqueeze(0)

    def get_seq_len(self, seq_len):
        return torch.ceil(seq_len.float() / self.hop_length).to(dtype=torch.long)

    def forward(self, input_signal, length):
        if self.dither > 0:
            input_signal += self.dither * torch.randn_like(input_signal)      # features.py:250-251
        mel, seq = stages.melspec(self._get_handle(), input_signal, length)
        if self.pad_to > 0 and mel.shape[-1] % self.pad_to:
            mel = torch.nn.functional.pad(mel, (0, self.pad_to - mel.shape[-1] % self.pad_to), value=self._desc.get("pad_value", 0.0))
        return mel, seq


def crop_or_pad_split(audio_length, image_len):
    """(pad_left, pad_right) of CropOrPadSpectrogramAugmentation's pad branch (audio_preprocessing.py:700-707): the odd frame
    goes on the right."""
    d = int(audio_length) - int(image_len)
    if d < 0:
        raise ValueError(f"{image_len} frames are cropped to {audio_length}, not padded")
    return d // 2, d - d // 2


class CropOrPadSpectrogramAugmentation(NonTrainableNM):
    """nemo/collections/asr/audio_preprocessing.py:666-738: pad or crop the spectrogram to ``audio_length`` frames.

    A wider batch tensor is cut per row at an offset drawn with the reference's own call on the default CPU generator,
    ``torch.randint(low=0, high=image_len - audio_length + 1, size=[num_images])`` -- after ``torch.manual_seed(s)`` this module
    crops where the reference crops; any other tensor is centred between zero frames (``crop_or_pad_split``)."""

    @property
    def input_ports(self):
        return {"input_signal": NeuralType(("B", "D", "T"), SpectrogramType()),
                "length": NeuralType(tuple("B"), LengthsType())}

    @property
    def output_ports(self):
        return {"processed_signal": NeuralType(("B", "D", "T"), SpectrogramType()),
                "processed_length": NeuralType(tuple("B"), LengthsType())}

    def __init__(self, audio_length, **kwargs):
        super().__init__()
        self.audio_length = audio_length

    def draw_offsets(self, num_images, image_len):
        """The reference's draw (:691); None when the tensor is not wider than audio_length (no draw happens there)."""
        if image_len <= self.audio_length:
            return None
        return torch.randint(low=0, high=image_len - self.audio_length + 1, size=[num_images])

    @torch.no_grad()
    def forward(self, input_signal, length):
        offsets = self.draw_offsets(input_signal.shape[0], input_signal.shape[-1])
        image, out_len = stages.crop_or_pad(input_signal, self.audio_length, offsets)
        return image, out_len.to(device=length.device, dtype=(length * 0 + self.audio_length).dtype)


def _resolved(a, w, n):
    """``[a : a + w]`` on an axis of n cells as Python (and torch) resolve it, negative starts included -> (lo, hi), lo <= hi."""
    lo, hi, _ = slice(a, a + w).indices(n)
    return lo, max(hi, lo)


def _check_spec(x):
    """Refuses anything but a contiguous float32 [B, D, T] device tensor -- before a generator is consumed."""
    if not torch.is_tensor(x) or x.device.type != "cuda":
        raise _lib.VasrError("viet-asr_amd kernels need HIP-resident tensors; there is no CPU fallback for this path")
    if x.dtype != torch.float32 or x.dim() != 3 or not x.is_contiguous():
        raise ValueError("the spectrogram must be a contiguous float32 [B, D, T] cuda tensor")


def _csr(rows):
    """Per-row rectangle lists -> (rects int32 [n, 4], row_begin int32 [len(rows) + 1]), empty rectangles dropped."""
    import numpy as np
    rows = [[r for r in row if r[0] < r[1] and r[2] < r[3]] for row in rows]
    begin = np.zeros(len(rows) + 1, dtype=np.int32)
    begin[1:] = np.cumsum([len(row) for row in rows])
    flat = [r for row in rows for r in row]
    return np.asarray(flat, dtype=np.int32).reshape(-1, 4), begin


class _RowMasks(nn.Module):
    """What SpecAugment and SpecCutout share: ``forward`` draws every batch row's rectangles (``draw_row``, the subclass's) and
    returns a new tensor with them zeroed (stages.spec_mask, the out-of-place kernel); the input is not modified."""

    @torch.no_grad()
    def forward(self, x):
        _check_spec(x)
        return stages.spec_mask(x, *_csr([self.draw_row(x.shape[1], x.shape[2]) for _ in range(x.shape[0])]))


class SpecAugment(_RowMasks):
    """nemo/collections/asr/parts/spectr_augment.py:7-56: ``freq_masks`` bands of up to ``freq_width`` feature rows and
    ``time_masks`` stretches of up to ``time_width`` frames set to zero, per batch row.  The draws are the reference's, call for
    call (``int(rng.uniform(0, hi))``: truncation towards zero, ``hi`` negative where the tensor is narrower than the width,
    negative starts resolved as slices); the zeros are written on the device."""

    def __init__(self, freq_masks=0, time_masks=0, freq_width=10, time_width=10, rng=None):
        super().__init__()
        import random
        self._rng = random.Random() if rng is None else rng
        self.freq_masks, self.time_masks = freq_masks, time_masks
        self.freq_width, self.time_width = freq_width, time_width

    def draw_row(self, feat, frames):
        """One batch row's draws -> its rectangles (f0, f1, t0, t1)."""
        out = []
        for _ in range(self.freq_masks):
            x_left = int(self._rng.uniform(0, feat - self.freq_width))
            w = int(self._rng.uniform(0, self.freq_width))
            out.append(_resolved(x_left, w, feat) + (0, frames))
        for _ in range(self.time_masks):
            y_left = int(self._rng.uniform(0, frames - self.time_width))
            w = int(self._rng.uniform(0, self.time_width))
            out.append((0, feat) + _resolved(y_left, w, frames))
        return out


class SpecCutout(_RowMasks):
    """nemo/collections/asr/parts/spectr_augment.py:59-97: ``rect_masks`` rectangles set to zero per batch row.  As in the
    reference the two widths are swapped against their names: the feature range is ``rect_x + U(0, rect_time)`` wide, the frame
    range ``rect_y + U(0, rect_freq)``."""

    def __init__(self, rect_masks=0, rect_time=5, rect_freq=20, rng=None):
        super().__init__()
        import random
        self._rng = random.Random() if rng is None else rng
        self.rect_masks, self.rect_time, self.rect_freq = rect_masks, rect_time, rect_freq

    def draw_row(self, feat, frames):
        out = []
        for _ in range(self.rect_masks):
            rect_x = int(self._rng.uniform(0, feat - self.rect_freq))
            rect_y = int(self._rng.uniform(0, frames - self.rect_time))
            w_x = int(self._rng.uniform(0, self.rect_time))
            w_y = int(self._rng.uniform(0, self.rect_freq))
            out.append(_resolved(rect_x, w_x, feat) + _resolved(rect_y, w_y, frames))
        return out


class SpectrogramAugmentation(NonTrainableNM):
    """nemo/collections/asr/audio_preprocessing.py:522-608: SpecCutout over the whole batch, then SpecAugment over the whole
    batch; the cutout exists only if ``rect_masks > 0``, the augment only if ``freq_masks + time_masks > 0``; one shared
    generator when ``rng`` is given, two independent unseeded ones when it is None.  A part that does not exist is the
    identity callable ``lambda x: x`` in ``spec_cutout`` / ``spec_augment``, as in the reference.  The tensor's width is T
    for every row (lengths are ignored), the input is not modified.

    ``draw`` is the host half -- the reference's draws, resolved to rectangles --, ``forward`` uploads them and runs the
    out-of-place kernel (vasr_spec_mask_f32).  The engines take an instance as ``spec_augment=`` and apply the same
    rectangles in place between the front end and the encoder (``engine.QuartzNetCTC.forward``)."""

    @property
    def input_ports(self):
        return {"input_spec": NeuralType(("B", "D", "T"), SpectrogramType())}

    @property
    def output_ports(self):
        return {"augmented_spec": NeuralType(("B", "D", "T"), SpectrogramType())}

    def __init__(self, freq_masks=0, time_masks=0, freq_width=10, time_width=10, rect_masks=0, rect_time=5, rect_freq=20,
                 rng=None):
        super().__init__()
        self.spec_cutout = self.spec_augment = lambda x: x
        if rect_masks > 0:
            self.spec_cutout = SpecCutout(rect_masks=rect_masks, rect_time=rect_time, rect_freq=rect_freq, rng=rng)
        if freq_masks + time_masks > 0:
            self.spec_augment = SpecAugment(freq_masks=freq_masks, time_masks=time_masks, freq_width=freq_width,
                                            time_width=time_width, rng=rng)

    def draw(self, batch, feat, frames, row_frames=None):
        """The rectangles of one ``forward`` on a [batch, feat, frames] tensor -> (rects int32 [n, 4] = (f0, f1, t0, t1), half-open
        and resolved; row_begin int32 [batch + 1]).  Host only.  The generators are consumed exactly as the reference's forward
        consumes them: the cutout's draws for every row, then the augment's for every row.

        row_frames (a list of ``batch`` frame counts): row b is drawn as a batch-1 forward on a [1, feat, row_frames[b]] tensor
        would draw it -- cutout then augment, row after row -- which is what ``row_independent=True`` of the engines needs."""
        rows = [[] for _ in range(batch)]
        parts = [mod for mod in (self.spec_cutout, self.spec_augment) if isinstance(mod, _RowMasks)]
        if row_frames is None:
            for mod in parts:
                for b in range(batch):
                    rows[b] += mod.draw_row(feat, frames)
        else:
            if len(row_frames) != batch:
                raise ValueError(f"row_frames needs one frame count per row ({batch}), got {len(row_frames)}")
            for b in range(batch):
                for mod in parts:
                    rows[b] += mod.draw_row(feat, int(row_frames[b]))
        return _csr(rows)

    @torch.no_grad()
    def forward(self, input_spec):
        _check_spec(input_spec)
        return stages.spec_mask(input_spec, *self.draw(*input_spec.shape))


class MultiplyBatch(NonTrainableNM):
    """nemo/collections/asr/audio_preprocessing.py:611-663: every element of the batch ``mult_batch`` times, so that later
    augmentations draw differently for each copy.  Four ``.repeat`` calls on the tensors where they are; no kernel."""

    @property
    def input_ports(self):
        return {"in_x": NeuralType(("B", "D", "T"), SpectrogramType()), "in_x_len": NeuralType(tuple("B"), LengthsType()),
                "in_y": NeuralType(("B", "D", "T"), SpectrogramType()), "in_y_len": NeuralType(tuple("B"), LengthsType())}

    @property
    def output_ports(self):
        return {"out_x": NeuralType(("B", "D", "T"), SpectrogramType()), "out_x_len": NeuralType(tuple("B"), LengthsType()),
                "out_y": NeuralType(("B", "D", "T"), SpectrogramType()), "out_y_len": NeuralType(tuple("B"), LengthsType())}

    def __init__(self, mult_batch=1):
        super().__init__()
        self.mult = mult_batch

    @torch.no_grad()
    def forward(self, in_x, in_x_len, in_y, in_y_len):
        return (in_x.repeat(self.mult, 1, 1), in_x_len.repeat(self.mult), in_y.repeat(self.mult, 1),
                in_y_len.repeat(self.mult))


class _MaskedConvParams(nn.Module):
    """Parameter container with the reference's MaskedConv1d key layout (``.conv.weight``)."""

    def __init__(self, cin, cout, k, groups=1):
        super().__init__()
        self.conv = nn.Conv1d(cin, cout, k, groups=groups, bias=False)


class _SqueezeExciteParams(nn.Module):
    """Parameter container with SqueezeExcite's key layout (parts/jasper.py:152-168: ``.fc.0.weight``, ``.fc.2.weight``)."""

    def __init__(self, channels, reduction_ratio):
        super().__init__()
        self.fc = nn.Sequential(nn.Linear(channels, channels // reduction_ratio, bias=False), nn.Identity(),
                                nn.Linear(channels // reduction_ratio, channels, bias=False))


class _JasperBlockParams(nn.Module):
    """ModuleList skeleton of one JasperBlock (parts/jasper.py:214-288): same indices, parameters only.  se: the
    SqueezeExcite reduction ratio (0: none); groups: of the main-branch convs, each followed by a GroupShuffle slot when > 1;
    heads: rows of the shared depthwise weights (-1: none); norm: GroupNorm's group count in every norm slot (0: BatchNorm)."""

    def __init__(self, inplanes, planes, repeat, kernel, separable, residual, residual_panes=(), se=0, groups=1, heads=-1,
                 norm=0):
        super().__init__()

        def norm_layer():   # parts/jasper.py:385-393
            return nn.GroupNorm(norm, planes) if norm else nn.BatchNorm1d(planes, eps=1e-3, momentum=0.1)

        layers, c = [], inplanes
        for r in range(repeat):
            if separable:
                dw = _MaskedConvParams(heads, heads, kernel, groups=heads) if heads != -1 else _MaskedConvParams(c, c, kernel, groups=c)
                layers += [dw, _MaskedConvParams(c, planes, 1, groups=groups)]
            else:
                layers += [_MaskedConvParams(c, planes, kernel, groups=groups)]
            layers.append(norm_layer())
            if groups > 1:
                layers.append(nn.Identity())                  # GroupShuffle slot (parts/jasper.py:396-399)
            if r != repeat - 1:
                layers += [nn.Identity(), nn.Identity()]      # activation, dropout slots
            if se and not residual:
                layers.append(_SqueezeExciteParams(planes, se))
            c = planes
        self.mconv = nn.ModuleList(layers)
        self.res = None
        if residual:   # one 1x1 conv + BN (+ SE) per pane (parts/jasper.py:264-288); no dense panes: the block input alone
            self.res = nn.ModuleList([nn.ModuleList([_MaskedConvParams(ip, planes, 1), norm_layer()]
                                                    + ([_SqueezeExciteParams(planes, se)] if se else []))
                                      for ip in (list(residual_panes) or [inplanes])])


def _init_weights(m, mode="xavier_uniform"):
    """parts/jasper.py:28-49."""
    if isinstance(m, (nn.Conv1d, nn.Linear)):
        init = {"xavier_uniform": lambda w: nn.init.xavier_uniform_(w, gain=1.0),
                "xavier_normal": lambda w: nn.init.xavier_normal_(w, gain=1.0),
                "kaiming_uniform": lambda w: nn.init.kaiming_uniform_(w, nonlinearity="relu"),
                "kaiming_normal": lambda w: nn.init.kaiming_normal_(w, nonlinearity="relu")}
        if mode not in init:
            raise ValueError("Unknown Initialization mode: {0}".format(mode))
        init[mode](m.weight)
    elif isinstance(m, nn.BatchNorm1d):
        m.running_mean.zero_()
        m.running_var.fill_(1)
        m.num_batches_tracked.zero_()
        nn.init.ones_(m.weight)
        nn.init.zeros_(m.bias)


class _HipWeights:
    """Mixin: keeps a libvasr handle in sync with the module's state_dict (re-packed after any load)."""

    def _invalidate(self):
        self._handle = None

    def load_state_dict(self, state_dict, strict=True):
        r = nn.Module.load_state_dict(self, state_dict, strict=strict)
        self._invalidate()
        return r


class JasperEncoder(_HipWeights, TrainableNM):
    """nemo/collections/asr/jasper.py:17-204."""

    @property
    def input_ports(self):
        return {"audio_signal": NeuralType(("B", "D", "T"), SpectrogramType()),
                "length": NeuralType(tuple("B"), LengthsType())}

    @property
    def output_ports(self):
        return {"outputs": NeuralType(("B", "D", "T"), AcousticEncodedRepresentation()),
                "encoded_lengths": NeuralType(tuple("B"), LengthsType())}

    def __init__(self, jasper, activation, feat_in, normalization_mode="batch", residual_mode="add", norm_groups=-1,
                 conv_mask=True, frame_splicing=1, init_mode="xavier_uniform"):
        super().__init__()
        if frame_splicing != 1:
            raise NotImplementedError("implemented: conv_mask=True, frame_splicing=1")
        # one activation for every block, as the reference's one module (jasper.py:150); unknown names: KeyError.  Unknown
        # normalization modes and group counts that do not divide a block's filters: ValueError, as the reference raises
        self._enc = enc = handle_arguments(dict(jasper=jasper, activation=activation, normalization_mode=normalization_mode,
                                                residual_mode=residual_mode, norm_groups=norm_groups, conv_mask=conv_mask),
                                           feat_in)
        self._act, self._res_mode, blocks = enc["activation"], enc["residual_mode"], enc["blocks"]
        check_dense_layout(blocks, feat_in)
        for b in blocks:
            if b["stride"] > 1 and b["dilation"] > 1:
                raise ValueError("Only stride OR dilation may be greater than 1")   # parts/jasper.py:61-62
        layers, c = [], feat_in
        residual_panes = []     # ONE list shared by the dense blocks, copied by each (jasper.py:152-161, parts/jasper.py:264)
        for b, se, (groups, heads), norm in zip(blocks, enc["se"], enc["groups"], enc["norm"]):
            k = odd_kernel(b["kernel"])
            dense_res = []
            if b["residual_dense"]:
                residual_panes.append(c)
                dense_res = residual_panes
            layers.append(_JasperBlockParams(c, b["filters"], b["repeat"], k, bool(b["separable"]), bool(b["residual"]),
                                             list(dense_res), se, groups, heads, norm))
            c = b["filters"]
        self.encoder = nn.Sequential(*layers)
        self._c_out = c
        self.apply(lambda m: _init_weights(m, mode=init_mode))
        self._handle = None

    def _get_handle(self):
        if self._handle is None:
            if not torch.cuda.is_available():
                raise _no_gpu()
            h = _lib.Handle(**self._enc)
            h.load_state_dict(self.state_dict())
            h.finalize()
            self._handle = h
        return self._handle

    def forward(self, audio_signal, length=None):
        if length is None:
            length = torch.full((audio_signal.shape[0],), audio_signal.shape[2], dtype=torch.int64,
                                device=audio_signal.device)
            return stages.encoder(self._get_handle(), audio_signal, length, self._c_out)[0]
        return stages.encoder(self._get_handle(), audio_signal, length, self._c_out)


class JasperDecoderForCTC(_HipWeights, TrainableNM):
    """nemo/collections/asr/jasper.py:207-254."""

    @property
    def input_ports(self):
        return {"encoder_output": NeuralType(("B", "D", "T"), AcousticEncodedRepresentation())}

    @property
    def output_ports(self):
        return {"output": NeuralType(("B", "T", "D"), LogprobsType())}

    def __init__(self, feat_in, num_classes, init_mode="xavier_uniform"):
        super().__init__()
        self._feat_in = feat_in
        self._num_classes = num_classes + 1          # + blank
        self.decoder_layers = nn.Sequential(nn.Conv1d(self._feat_in, self._num_classes, kernel_size=1, bias=True))
        self.apply(lambda m: _init_weights(m, mode=init_mode))
        self._handle = None

    def _get_handle(self):
        if self._handle is None:
            if not torch.cuda.is_available():
                raise _no_gpu()
            h = _lib.Handle(dec_feat_in=self._feat_in, num_classes=self._num_classes)
            h.load_state_dict(self.state_dict())
            h.finalize()
            self._handle = h
        return self._handle

    def forward(self, encoder_output):
        return stages.decoder(self._get_handle(), encoder_output)


class JasperDecoderForClassification(_HipWeights, TrainableNM):
    """nemo/collections/asr/jasper.py:257-319: pooling over time, a Linear layer, optionally a softmax."""

    @property
    def input_ports(self):
        return {"encoder_output": NeuralType(("B", "D", "T"), AcousticEncodedRepresentation())}

    @property
    def output_ports(self):
        return {"logits": NeuralType(("B", "D"), LogitsType())}

    def __init__(self, *, feat_in, num_classes, init_mode="xavier_uniform", return_logits=True, pooling_type='avg', **kwargs):
        super().__init__()
        self._feat_in = feat_in
        self._return_logits = return_logits
        self._num_classes = num_classes
        if pooling_type not in ("avg", "max"):
            raise ValueError('Pooling type chosen is not valid. Must be either `avg` or `max`')
        self._pooling = 0 if pooling_type == "avg" else 1
        self.decoder_layers = nn.Sequential(nn.Linear(self._feat_in, self._num_classes, bias=True))
        self.apply(lambda m: _init_weights(m, mode=init_mode))
        self._handle = None

    def _get_handle(self):
        if self._handle is None:
            if not torch.cuda.is_available():
                raise _no_gpu()
            h = _lib.Handle(classifier=(self._feat_in, self._num_classes, self._pooling))
            h.load_state_dict(self.state_dict())
            h.finalize()
            self._handle = h
        return self._handle

    def forward(self, encoder_output):
        return stages.classifier(self._get_handle(), encoder_output, softmax=not self._return_logits)


class GreedyCTCDecoder(TrainableNM):
    """nemo/collections/asr/greedy_ctc_decoder.py:9-36."""

    @property
    def input_ports(self):
        return {"log_probs": NeuralType(("B", "T", "D"), LogprobsType())}

    @property
    def output_ports(self):
        return {"predictions": NeuralType(("B", "T"), PredictionsType())}

    def __init__(self):
        super().__init__()

    def forward(self, log_probs):
        return stages.greedy_argmax(log_probs)


class CTCLossNM(NonTrainableNM):
    """nemo/collections/asr/losses.py:10-61, forward only: the loss an evaluation reports next to WER and CER
    (``Evaluation_Loss``, helpers.py:146-204).  num_classes: the number of labels without the blank, which is id
    ``num_classes``.  ``forward`` returns the reference's ``torch.mean(loss)`` of the per-row ``nn.CTCLoss(reduction='none')``
    values -- not divided by the target lengths -- as a 0-dim float32 device tensor (``stages.ctc_loss``,
    vasr_ctc_loss_f32).  The result carries no graph: there is no backward pass, training stays out of scope (DESIGN.md
    section 8)."""

    @property
    def input_ports(self):
        return {"log_probs": NeuralType(("B", "T", "D"), LogprobsType()),
                "targets": NeuralType(("B", "T"), LabelsType()),
                "input_length": NeuralType(tuple("B"), LengthsType()),
                "target_length": NeuralType(tuple("B"), LengthsType())}

    @property
    def output_ports(self):
        return {"loss": NeuralType(elements_type=LossType())}

    def __init__(self, num_classes):
        super().__init__()
        self._blank = int(num_classes)

    def forward(self, log_probs, targets, input_length, target_length):
        return stages.ctc_loss(log_probs, input_length, targets, target_length, self._blank).mean(dtype=torch.float32)


class BeamSearchDecoderWithLM(NonTrainableNM):
    """nemo/collections/asr/beam_search_decoder.py:14-102 (pyctcdecode-backed in the reference).

    The prefix beam search (with optional n-gram LM) lives in beam.py; unlike the reference it
    accepts any batch size and stays on the device.  ``forward`` returns the best string for B == 1
    (what infer.py consumes: evaluated_tensors[0][0]) and a list of strings otherwise.
    """

    @property
    def input_ports(self):
        return {"log_probs": NeuralType(("B", "T", "D"), LogprobsType()),
                "log_probs_length": NeuralType(tuple("B"), LengthsType())}

    @property
    def output_ports(self):
        return {"predictions": NeuralType(("B", "T"), PredictionsType())}

    def __init__(self, lm_path, vocab, beam_width, alpha, beta, num_cpus=1, cutoff_prob=1.0, cutoff_top_n=40,
                 input_tensor=True, allow_missing_lm=False, unigrams="auto"):
        """unigrams (net-new): "auto" = what build_ctcdecoder does for lm_path's suffix -- the ARPA's own unigram list + character
        trie for "*.arpa", none otherwise --, None = no unigram list on any file (the behaviour the reference got from its
        `.binary`), or a list of words (viet_asr_amd/beam.py)."""
        super().__init__()
        if self._factory is not None and self._factory.world_size > 1:
            raise ValueError("BeamSearchDecoderWithLM does not run in distributed mode")   # :79-80
        from .beam import BeamSearchDecoder
        self.vocab, self.beam_width = list(vocab), beam_width
        # an lm_path that cannot be read (KenLM binaries, a missing file) raises unless allow_missing_lm (beam.LM_HELP)
        self.decoder = BeamSearchDecoder(self.vocab, lm_path=lm_path, alpha=alpha, beta=beta, allow_missing_lm=allow_missing_lm,
                                         unigrams=unigrams)
        self.num_cpus, self.cutoff_prob, self.cutoff_top_n, self.input_tensor = num_cpus, cutoff_prob, cutoff_top_n, \
            input_tensor

    def forward(self, log_probs, log_probs_length=None):
        # Batch 1 (all the reference accepts, :96) searches every frame, like pyctcdecode on log_probs[0].  In a padded
        # batch the shorter rows' trailing frames hold the head's output on masked input, not blanks: each row is
        # searched over its own log_probs_length[b] frames (float lengths from the encoder, quirk Q3, truncated).
        frames = None
        if log_probs.shape[0] > 1 and log_probs_length is not None:
            frames = torch.as_tensor(log_probs_length).to(torch.float64).floor().clamp(0, log_probs.shape[1]).to(torch.int32)
        texts = self.decoder.decode_batch(log_probs, beam_width=self.beam_width, frames=frames)
        return texts[0] if len(texts) == 1 else texts


class AudioDataLayer(DataLayerNM):
    """Batched counterpart of infer.py:16-54: a one-shot iterator over (audio_signal [B,L], a_sig_length [B]).

    ``set_signal(x)`` keeps the reference's single-utterance call; ``set_batch(list)`` zero-pads to the
    longest utterance like ``seq_collate_fn`` (parts/dataset.py:14-53).
    """

    @property
    def output_ports(self):
        return {"audio_signal": NeuralType(("B", "T"), AudioSignal(freq=self._sample_rate)),
                "a_sig_length": NeuralType(tuple("B"), LengthsType())}

    def __init__(self, sample_rate):
        super().__init__()
        self._sample_rate = sample_rate
        self.output = False
        self.signal = self.signal_shape = None

    def set_signal(self, signal):
        """The reference's single-utterance call (infer.py:29-33): a batch of one."""
        import numpy as np
        self.set_batch([np.asarray(signal, dtype=np.float32).reshape(-1)])

    def set_batch(self, signals):
        import numpy as np
        # cast first: this layer takes samples as they are (infer.py:29-33 hands it floats) -- integer input is NOT scaled
        # by 2^-15 here, as the engines' PCM ingest scales it
        batch, lens = collate([np.asarray(s, dtype=np.float32) for s in signals])
        self.signal, self.signal_shape, self.output = batch, np.array(lens, dtype=np.int64), True

    def __iter__(self):
        return self

    def __next__(self):
        if not self.output:
            raise StopIteration
        self.output = False
        return torch.as_tensor(self.signal, dtype=torch.float32), torch.as_tensor(self.signal_shape, dtype=torch.int64)

    def __len__(self):
        return 1

    @property
    def dataset(self):
        return None

    @property
    def data_iterator(self):
        return self
