"""The encoder's conv chain as arithmetic on lengths: pure functions of the block descriptions ``engine.blocks_from_config``
returns.  Nothing here touches the library or a device; the engines' ``frames_of``, ``frame_seconds``, ``halo_mel_frames``
and ``_encoded_length`` are calls into this module.

Two chains run over the same steps and are different things:
  * ``frames_of`` is what the kernels do: whole frames, ``(t - shrink) // stride + 1`` per conv, from ``1 + samples // hop``;
  * ``encoded_length`` is what the reference REPORTS (MaskedConv1d.get_seq_len, quirk Q3): a float division per conv, both
    convs of a separable sub-block, truncated between convs, from the front end's ``seq``.
For one and the same row they legitimately give 501 and 500.0.
"""
from collections import namedtuple

import numpy as np


def odd_kernel(kernel):
    """The kernel a conv really has: an even one grows by one tap (parts/jasper.py:52-57 for ``kernel_size_factor``; the
    library does the same to every even kernel it is given)."""
    return kernel + 1 if kernel % 2 == 0 else kernel


class ConvStep(namedtuple("ConvStep", "kernel stride dilation pad")):
    """One MaskedConv1d of the chain: the effective (odd) kernel, stride, dilation and the padding JasperBlock gives it
    (get_same_padding, parts/jasper.py:60-65)."""
    __slots__ = ()

    @property
    def shrink(self):
        """What the conv takes off a length before its stride divides: out = (length - shrink) // stride + 1."""
        return self.dilation * (self.kernel - 1) + 1 - 2 * self.pad

    @property
    def reach(self):
        """Input frames the conv sees on either side of an output frame; 0: the step does not widen the receptive field."""
        return (self.kernel - 1) // 2 * self.dilation


def conv_steps(blocks):
    """Every conv that changes a length or widens the receptive field, in order: per block ``repeat`` times its K-tap conv
    (the depthwise one of a separable block) and, behind a depthwise conv, the 1x1 that completes the sub-block."""
    for b in blocks:
        k = odd_kernel(b["kernel"])
        pad = (b["dilation"] * k) // 2 - 1 if b["dilation"] > 1 else k // 2
        for _ in range(b["repeat"]):
            yield ConvStep(k, b["stride"], b["dilation"], pad)
            if b["separable"]:
                yield ConvStep(1, 1, 1, 0)


def stride_product(blocks):
    """Mel frames per encoded frame."""
    rate = 1
    for s in conv_steps(blocks):
        rate *= s.stride
    return rate


def frames_of(blocks, hop, length):
    """The encoded frames of each row alone for a [B] int64 tensor of sample counts, on its device: the conv chain of
    vasr_encoded_frames in integer tensor ops -> [B] int32."""
    import torch        # (here only: the rest of the module, and synth.py which uses it, is numpy alone)
    t = 1 + torch.div(length, hop, rounding_mode="floor")
    for s in conv_steps(blocks):
        if (s.shrink, s.stride) != (1, 1):          # (a 1x1 conv keeps every length: no launches for it)
            t = torch.div(t - s.shrink, s.stride, rounding_mode="floor") + 1
    return t.to(torch.int32)


def encoded_length(blocks, seq):
    """MaskedConv1d.get_seq_len chain (jasper.py:108-111, quirk Q3) on the host: float result, truncated between convs."""
    lf = float(seq)
    for s in conv_steps(blocks):
        lf = float(np.float32(np.float32(int(lf) - s.shrink) / np.float32(s.stride)) + np.float32(1.0))
    return lf


def halo_mel_frames(blocks):
    """Half-width of the encoder's receptive field in mel frames (even): the sum over the convs of their reach times the
    stride product in front of each."""
    if any(b["stride"] > 1 and b["repeat"] > 1 for b in blocks):
        raise NotImplementedError("strided block with repeat > 1")
    h, rate = 0, 1
    for s in conv_steps(blocks):
        h += s.reach * rate
        rate *= s.stride
    return h + (h & 1)
