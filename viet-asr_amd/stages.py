"""Per-stage wrappers over the C ABI: torch tensors in, torch tensors out, on the current stream.

Each function is the forward of one reference NeuralModule (ports and dtypes as in
SURVEY.md §8b); asr.py's module classes call these.  Result tensors are allocated here with
torch (caching allocator); the library only fills them.
"""
import torch

from . import _lib


def _st():
    return torch.cuda.current_stream().cuda_stream


def _need_cuda(*ts):
    for t in ts:
        if t.device.type != "cuda":
            raise _lib.VasrError("viet-asr_amd kernels need HIP-resident tensors (got a CPU tensor); "
                                 "there is no CPU fallback for this path")


# One workspace per (device, STREAM): the library is re-entrant per handle + stream (include/vasr.h), so two host threads
# driving per-module calls on two streams must not be handed the same scratch memory (rounds 1-5 kept one per device).
# Allocated while its stream is current, so the caching allocator's stream-ordered reuse covers a replaced (grown) buffer.
_ws_cache = {}
_ws_lock = __import__("threading").Lock()


def _workspace(device, nbytes):
    key = (device, _st())
    with _ws_lock:
        ws = _ws_cache.get(key)
        if ws is None or ws.numel() < nbytes:
            _ws_cache[key] = None
            ws = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=device)
            _ws_cache[key] = ws
        return ws


def melspec(handle, input_signal, length):
    """AudioToMelSpectrogramPreprocessor.forward -> (processed_signal [B,64,T] f32, processed_length [B] i64)."""
    _need_cuda(input_signal, length)
    x = input_signal.to(torch.float32).contiguous()
    ln = length.to(torch.int64).contiguous()
    B, L = x.shape
    T = handle.mel_frames(L)
    mel = torch.empty((B, 64, T), dtype=torch.float32, device=x.device)
    seq = torch.empty((B,), dtype=torch.int64, device=x.device)
    _lib.check(_lib.lib().vasr_melspec_f32(handle.h, x.data_ptr(), ln.data_ptr(), B, L, mel.data_ptr(),
                                           seq.data_ptr(), _st()))
    return mel, seq


def encoder(handle, audio_signal, length, c_out):
    """JasperEncoder.forward -> (outputs [B,C,T'] f32, encoded_lengths [B] f32)."""
    _need_cuda(audio_signal, length)
    x = audio_signal.to(torch.float32).contiguous()
    ln = length.to(torch.int64).contiguous()
    B, _, T = x.shape
    T1 = handle.encoded_frames(T)
    out = torch.empty((B, c_out, T1), dtype=torch.float32, device=x.device)
    enc_len = torch.empty((B,), dtype=torch.float32, device=x.device)
    ws = _workspace(x.device, handle.workspace_bytes(B, mel_frames=T))
    _lib.check(_lib.lib().vasr_encoder_f32(handle.h, x.data_ptr(), ln.data_ptr(), B, T, out.data_ptr(),
                                           enc_len.data_ptr(), ws.data_ptr(), ws.numel(), _st()))
    return out, enc_len


def decoder(handle, encoder_output):
    """JasperDecoderForCTC.forward -> log_probs [B,T',V+1] f32."""
    _need_cuda(encoder_output)
    x = encoder_output.to(torch.float32).contiguous()
    B, C, T1 = x.shape
    V = handle.num_classes
    ld = int(_lib.lib().vasr_padded_frames(T1))
    need = ((B * C * ld * 4 + 255) // 256) * 256 + B * V * ld * 4
    need = ((need + 255) // 256) * 256 + B * 1024       # + the maxima table of the port tensor (fp16-split head, vasr.h)
    ws = _workspace(x.device, need)
    logp = torch.empty((B, T1, V), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().vasr_decoder_logsoftmax_f32(handle.h, x.data_ptr(), B, T1, logp.data_ptr(),
                                                      ws.data_ptr(), ws.numel(), _st()))
    return logp


def crop_or_pad(input_signal, audio_length, offsets=None):
    """CropOrPadSpectrogramAugmentation.forward -> (processed_signal [B,D,audio_length] f32, processed_length [B] i64).
    offsets [B] i64 (any device): where each row is cut when it is wider than audio_length."""
    _need_cuda(input_signal)
    x = input_signal.to(torch.float32).contiguous()
    B, D, T = x.shape
    A = int(audio_length)
    if T > A and offsets is None:
        raise ValueError(f"{T} frames are cropped to {A}: offsets needed")
    off = None if offsets is None else torch.as_tensor(offsets).to(device=x.device, dtype=torch.int64).contiguous()
    if off is not None and off.shape != (B,):
        raise ValueError(f"offsets must have shape ({B},), got {tuple(off.shape)}")
    out = torch.empty((B, D, A), dtype=torch.float32, device=x.device)
    out_len = torch.empty((B,), dtype=torch.int64, device=x.device)
    _lib.check(_lib.lib().vasr_crop_or_pad_f32(x.data_ptr(), B, D, T, A, off.data_ptr() if off is not None else None,
                                               out.data_ptr(), out_len.data_ptr(), _st()))
    return out, out_len


def _feature_pitch(t, what):
    """The row pitch of a [B, D, T] float32 tensor whose feature rows are equally spaced: a contiguous tensor (pitch T) or a
    column slice ``wide[:, :, :T]`` of one (pitch: wide's width)."""
    if t.dtype != torch.float32 or t.dim() != 3 or 0 in t.shape:
        raise ValueError(f"{what} must be a non-empty [B, D, T] float32 tensor")
    B, D, T = t.shape
    if t.is_contiguous():
        return T
    ld = t.stride(1)
    if t.stride(2) != 1 or ld < T or t.stride(0) != D * ld:
        raise ValueError(f"{what} must be contiguous, or a column slice of a contiguous [B, D, ld] tensor")
    return ld


def upload_masks(rects, row_begin, device):
    """Host rectangles [n, 4] and row table [B + 1] (int32) -> the two device tensors, through ONE pinned staging buffer and one
    asynchronous copy on the current stream: nothing synchronises."""
    import numpy as np
    rects = np.ascontiguousarray(rects, dtype=np.int32).reshape(-1, 4)
    row_begin = np.ascontiguousarray(row_begin, dtype=np.int32).reshape(-1)
    head = (row_begin.size + 3) // 4 * 4
    host = torch.zeros(head + max(rects.size, 4), dtype=torch.int32).pin_memory()
    host[: row_begin.size] = torch.from_numpy(row_begin)
    host[head: head + rects.size] = torch.from_numpy(rects.reshape(-1))
    dev = host.to(device, non_blocking=True)
    return dev[head:].view(-1, 4), dev[: row_begin.size]


def spec_mask(input_spec, rects, row_begin, out=None):
    """SpecAugment / SpecCutout's ``x.masked_fill(mask, 0)`` for a mask that is a union of rectangles (vasr_spec_mask_f32): rects
    [n, 4] int32 = (f0, f1, t0, t1), half-open and resolved; row_begin [B + 1] int32, row b owns rects[row_begin[b] :
    row_begin[b + 1]] (both on the device already, or host arrays that are uploaded without synchronising).  -> a new
    contiguous tensor, or ``out``: ``out=input_spec`` selects the form that only stores zeros over the rectangles (and returns
    input_spec), any other ``out`` [B, D, T] receives the masked copy.  input_spec and out may be column slices of wider
    contiguous tensors: the columns behind T are never written.  One launch."""
    _need_cuda(input_spec)
    ld_in = _feature_pitch(input_spec, "input_spec")
    B, D, T = input_spec.shape
    if not (torch.is_tensor(rects) and torch.is_tensor(row_begin)):
        rects, row_begin = upload_masks(rects, row_begin, input_spec.device)
    _need_cuda(rects, row_begin)
    if rects.dtype != torch.int32 or row_begin.dtype != torch.int32 or not rects.is_contiguous() or not row_begin.is_contiguous():
        raise ValueError("rects and row_begin must be contiguous int32 tensors")
    if row_begin.numel() != B + 1 or rects.numel() % 4:
        raise ValueError(f"row_begin needs {B + 1} entries (got {row_begin.numel()}), rects four per rectangle")
    if out is None:
        out = torch.empty((B, D, T), dtype=torch.float32, device=input_spec.device)
    elif out is not input_spec:
        _need_cuda(out)
        if out.shape != input_spec.shape or out.device != input_spec.device:
            raise ValueError("out must have input_spec's shape and device")
    ld_out = _feature_pitch(out, "out")
    # (an empty device tensor has no address; with no rectangle at all the list pointer is never followed)
    rects_ptr = rects.data_ptr() if rects.numel() else row_begin.data_ptr()
    _lib.check(_lib.lib().vasr_spec_mask_f32(input_spec.data_ptr(), ld_in, out.data_ptr(), ld_out, B, D, T, rects_ptr,
                                             row_begin.data_ptr(), _st()))
    return out


def classifier(handle, encoder_output, softmax=False):
    """JasperDecoderForClassification.forward -> logits (or probabilities) [B,num_classes] f32."""
    _need_cuda(encoder_output)
    x = encoder_output.to(torch.float32).contiguous()
    B, C, T1 = x.shape
    ws = _workspace(x.device, B * C * 4)
    out = torch.empty((B, handle.num_classes), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().vasr_classifier_f32(handle.h, x.data_ptr(), B, T1, int(bool(softmax)), out.data_ptr(),
                                              ws.data_ptr(), ws.numel(), _st()))
    return out


def greedy_argmax(log_probs):
    """GreedyCTCDecoder.forward -> predictions [B,T'] i64."""
    _need_cuda(log_probs)
    x = log_probs.to(torch.float32).contiguous()
    B, T1, V = x.shape
    pred = torch.empty((B, T1), dtype=torch.int64, device=x.device)
    _lib.check(_lib.lib().vasr_greedy_argmax(x.data_ptr(), B, T1, V, pred.data_ptr(), _st()))
    return pred


def ctc_collapse(predictions, blank_id):
    """Device side of __ctc_decoder_predictions_tensor -> (ids [B,T'] i32, id_len [B] i32)."""
    _need_cuda(predictions)
    p = predictions.to(torch.int64).contiguous()
    B, T1 = p.shape
    ids = torch.empty((B, T1), dtype=torch.int32, device=p.device)
    n = torch.empty((B,), dtype=torch.int32, device=p.device)
    _lib.check(_lib.lib().vasr_ctc_collapse(p.data_ptr(), B, T1, int(blank_id), ids.data_ptr(), n.data_ptr(), _st()))
    return ids, n


def _space_array(space_ids):
    sp = [int(s) for s in space_ids]
    return (_lib.C.c_int32 * max(len(sp), 1))(*sp), len(sp)


def _i32_rows(t, dev):
    """-> (t as a contiguous int32 tensor on dev, the tensor whose data_ptr() to pass: a stand-in where t has no storage)"""
    x = t.to(device=dev, dtype=torch.int32).contiguous()
    return x, (x if x.numel() else torch.empty(1, dtype=torch.int32, device=dev))


def _pair_args(hyp_ids, hyp_len, ref_ids, ref_len, space_ids):
    """The arguments ``error_counts`` and ``error_ops`` share, checked and cast on the device -> (B, dev, h, hp, hn, r, rp, rn,
    arr, n_space): h / r the int32 id batches, hp / rp the tensors whose data_ptr() to pass (a [B, 0] tensor has no storage to
    point at: the library wants a pointer it never reads), hn / rn the int32 lengths, arr the host array of space ids."""
    _need_cuda(hyp_ids, hyp_len, ref_ids, ref_len)
    if hyp_ids.dim() != 2 or ref_ids.dim() != 2:
        raise ValueError(f"hyp_ids / ref_ids must be [B, T], got {tuple(hyp_ids.shape)} / {tuple(ref_ids.shape)}")
    B = hyp_ids.shape[0]
    if ref_ids.shape[0] != B or tuple(hyp_len.shape) != (B,) or tuple(ref_len.shape) != (B,):
        raise ValueError(f"batch sizes differ: ids {tuple(hyp_ids.shape)} / {tuple(ref_ids.shape)}, lengths "
                         f"{tuple(hyp_len.shape)} / {tuple(ref_len.shape)}")
    dev = hyp_ids.device
    (h, hp), (r, rp) = _i32_rows(hyp_ids, dev), _i32_rows(ref_ids, dev)
    hn, rn = hyp_len.to(torch.int32).contiguous(), ref_len.to(device=dev, dtype=torch.int32).contiguous()
    arr, ns = _space_array(space_ids)
    return B, dev, h, hp, hn, r, rp, rn, arr, ns


def error_counts(hyp_ids, hyp_len, ref_ids, ref_len, space_ids):
    """word_error_rate (metrics.py:30-63) per row, both use_cer settings -> counts [B,4] i32 =
    {word_edits, ref_words, char_edits, ref_chars} (vasr_error_counts_i32).  hyp_ids [B,Th] / hyp_len [B]: collapsed ids
    (greedy or beam); ref_ids [B,Tr] / ref_len [B]: the data layer's transcripts / transcript_length -- int64 is cast on
    the device.  space_ids: the label ids str.split() separates on (host integers, at most 8).  Enqueued on the current
    stream; nothing synchronises.  A row with a negative length comes back as four -1."""
    B, dev, h, hp, hn, r, rp, rn, arr, ns = _pair_args(hyp_ids, hyp_len, ref_ids, ref_len, space_ids)
    counts = torch.empty((B, 4), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().vasr_error_counts_i32(hp.data_ptr(), h.shape[1], hn.data_ptr(), rp.data_ptr(), r.shape[1],
                                                    rn.data_ptr(), B, arr, ns, counts.data_ptr(), _st()))
    return counts


def error_ops(hyp_ids, hyp_len, ref_ids, ref_len, space_ids, script=False):
    """``error_counts``' two distances split by the alignment rule of include/vasr.h (vasr_error_ops_i32) -> ops [B,8] i32 =
    {word_sub, word_del, word_ins, word_hits, char_sub, char_del, char_ins, char_hits}; with script=True ->
    (ops, script [B,L] i32, script_len [B] i32): the word-level edit script of every row, op codes 0 hit / 1 substitution /
    2 deletion / 3 insertion over script[b, :script_len[b]], L = (Th + 1) // 2 + (Tr + 1) // 2 (entries behind a length are
    not written); both widths must then be <= 1024 (NotImplementedError beyond).  Arguments as ``error_counts``.  Enqueued
    on the current stream; nothing synchronises.  A row with a negative length comes back as eight -1 (script_len -1)."""
    B, dev, h, hp, hn, r, rp, rn, arr, ns = _pair_args(hyp_ids, hyp_len, ref_ids, ref_len, space_ids)
    ops = torch.empty((B, 8), dtype=torch.int32, device=dev)
    steps = steps_len = None
    if script:
        steps = torch.empty((B, max(1, (h.shape[1] + 1) // 2 + (r.shape[1] + 1) // 2)), dtype=torch.int32, device=dev)
        steps_len = torch.empty((B,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().vasr_error_ops_i32(hp.data_ptr(), h.shape[1], hn.data_ptr(), rp.data_ptr(), r.shape[1],
                                                 rn.data_ptr(), B, arr, ns, ops.data_ptr(),
                                                 steps.data_ptr() if script else None,
                                                 steps_len.data_ptr() if script else None, _st()))
    return (ops, steps, steps_len) if script else ops


def nbest_error_counts(ids, id_len, count, ref_ids, ref_len, space_ids):
    """``error_counts`` of every slot of an n-best list against the row's one reference, and the best slot per row
    (vasr_nbest_error_counts_i32).  ids [B,N,T] / id_len [B,N] / count [B]: ``DeviceBeamDecoder.decode_beams_ids``' first
    three results; ref_ids [B,Tr] / ref_len [B]: the transcripts, one row per utterance.  -> dict(slot_counts [B,N,4] i32 --
    four -1 in the slots behind count --, counts [B,4] i32 = {min word_edits, ref_words, min char_edits, ref_chars} over the
    filled slots (``error_counts``' layout: it accumulates the same way), slot [B,2] i32: the slots of the two minima, the
    lower among equals).  A row that cannot be scored (a negative length, count < 1) is -1 throughout.  Enqueued on the
    current stream; nothing synchronises."""
    _need_cuda(ids, id_len, count, ref_ids, ref_len)
    if ids.dim() != 3 or ref_ids.dim() != 2:
        raise ValueError(f"ids must be [B, N, T] and ref_ids [B, T], got {tuple(ids.shape)} / {tuple(ref_ids.shape)}")
    B, N = ids.shape[0], ids.shape[1]
    if ref_ids.shape[0] != B or tuple(id_len.shape) != (B, N) or tuple(count.shape) != (B,) or tuple(ref_len.shape) != (B,):
        raise ValueError(f"shapes differ: ids {tuple(ids.shape)}, id_len {tuple(id_len.shape)}, count {tuple(count.shape)}, "
                         f"ref_ids {tuple(ref_ids.shape)}, ref_len {tuple(ref_len.shape)}")
    dev = ids.device
    (h, hp), (r, rp) = _i32_rows(ids, dev), _i32_rows(ref_ids, dev)
    hn, cn = id_len.to(torch.int32).contiguous(), count.to(torch.int32).contiguous()
    rn = ref_len.to(device=dev, dtype=torch.int32).contiguous()
    arr, ns = _space_array(space_ids)
    slot_counts = torch.empty((B, N, 4), dtype=torch.int32, device=dev)
    counts = torch.empty((B, 4), dtype=torch.int32, device=dev)
    slot = torch.empty((B, 2), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().vasr_nbest_error_counts_i32(hp.data_ptr(), h.shape[2], hn.data_ptr() if hn.numel() else None,
                                                          cn.data_ptr(), N, rp.data_ptr(), r.shape[1], rn.data_ptr(), B,
                                                          arr, ns, slot_counts.data_ptr() if N else None, counts.data_ptr(),
                                                          slot.data_ptr(), _st()))
    return dict(slot_counts=slot_counts, counts=counts, slot=slot)


def classification_scores(logits, targets=None, k=0, want_prob=False, want_loss=True):
    """Per-row scores of classification logits [B,C] (vasr_class_scores_f32) -> a dict with the requested tensors:
    ``rank`` [B] i32 and (unless want_loss=False, which spares the kernel its logsumexp pass) ``loss`` [B] f32 when ``targets`` [B] is given -- the target's 0-based position among the row's classes
    (top-k correct iff 0 <= rank < k; metrics.classification_accuracy, metrics.py:66-99) and
    nn.CrossEntropyLoss(reduction='none'); ``indices`` [B,k] i32 and ``values`` [B,k] f32 when k > 0 (1..16, k <= C), plus
    ``probs`` [B,k] f32, the softmax probabilities, with want_prob.  The order: larger value first, NaN above every number,
    the lower class index first among equal values (include/vasr.h).  A target outside [0, C) gives rank -1 and loss 0.
    logits: float32 cuda (other floating types are cast on the device); targets: any integer type, cast to int64 on the
    device.  Enqueued on the current stream; nothing synchronises."""
    _need_cuda(logits)
    if logits.dim() != 2:
        raise ValueError(f"logits must be [B, C], got {tuple(logits.shape)}")
    if not logits.dtype.is_floating_point:
        raise ValueError(f"logits must be floating point, got {logits.dtype}")
    B, Cn = logits.shape
    k = int(k)
    if targets is None and k == 0:
        raise ValueError("nothing requested: give targets, k > 0, or both")
    if want_prob and k == 0:
        raise ValueError("want_prob needs k > 0")
    dev = logits.device
    x = logits.to(torch.float32).contiguous()
    out, t = {}, None
    if targets is not None:
        if targets.dtype.is_floating_point or targets.dtype == torch.bool or tuple(targets.shape) != (B,):
            raise ValueError(f"targets must be {B} integers, got {targets.dtype} {tuple(targets.shape)}")
        t = targets.to(device=dev, dtype=torch.int64).contiguous()
        out["rank"] = torch.empty((B,), dtype=torch.int32, device=dev)
        if want_loss:
            out["loss"] = torch.empty((B,), dtype=torch.float32, device=dev)
    if k:
        out["indices"] = torch.empty((B, k), dtype=torch.int32, device=dev)
        out["values"] = torch.empty((B, k), dtype=torch.float32, device=dev)
        if want_prob:
            out["probs"] = torch.empty((B, k), dtype=torch.float32, device=dev)
    ptr = lambda name: out[name].data_ptr() if name in out else None  # noqa: E731
    with torch.cuda.device(dev):
        # (an empty batch or k out of range is refused by the library before anything is launched)
        _lib.check(_lib.lib().vasr_class_scores_f32(x.data_ptr() if x.numel() else None, B, Cn,
                                                    t.data_ptr() if t is not None and B else None, k, ptr("indices"),
                                                    ptr("values"), ptr("probs"), ptr("rank"), ptr("loss"), _st()))
    return out


def _i32_lengths(t, dev):
    """Lengths of any dtype -> int32 on dev.  Float lengths (the encoder's, quirk Q3) are truncated as ``.long()`` truncates
    them; values outside int32 are clamped so that a negative length stays negative and a huge one stays huge."""
    x = torch.as_tensor(t).to(device=dev)
    return x.to(torch.int64).clamp(-1, 2 ** 31 - 1).to(torch.int32).contiguous()


def ctc_loss(log_probs, input_length, targets, target_length, blank):
    """nn.CTCLoss(blank, reduction='none', zero_infinity=False) per row, as CTCLossNM builds it (vasr_ctc_loss_f32) -> loss
    [B] f32 on the device = -log P(targets[b, :target_length[b]] | log_probs[b, :input_length[b]]).  log_probs [B,T',C] f32
    cuda, batch first as the decoder delivers them (other floating types are cast on the device); input_length [B]: any
    dtype, float lengths from the encoder are truncated as ``CTCLossNM._loss``'s ``.long()`` truncates them; targets [B,W] /
    target_length [B]: the data layer's transcripts / transcript_length, W <= 4096 (NotImplementedError beyond).  +inf for a
    row without a path; a quiet NaN for a row with a negative length or with an id inside its length that is out of range
    or the blank (include/vasr.h).  Forward only: the result carries no graph.  Enqueued on the current stream; nothing
    synchronises."""
    _need_cuda(log_probs)
    if log_probs.dim() != 3 or not log_probs.dtype.is_floating_point:
        raise ValueError(f"log_probs must be a floating-point [B, T, C] tensor, got {log_probs.dtype} {tuple(log_probs.shape)}")
    if targets.dim() != 2:
        raise ValueError(f"targets must be [B, W], got {tuple(targets.shape)}")
    B, T1, Cn = log_probs.shape
    if targets.shape[0] != B or tuple(torch.as_tensor(input_length).shape) != (B,) or \
            tuple(torch.as_tensor(target_length).shape) != (B,):
        raise ValueError(f"batch sizes differ: log_probs {tuple(log_probs.shape)}, targets {tuple(targets.shape)}, lengths "
                         f"{tuple(torch.as_tensor(input_length).shape)} / {tuple(torch.as_tensor(target_length).shape)}")
    dev = log_probs.device
    x = log_probs.detach().to(torch.float32).contiguous()
    xp = x if x.numel() else torch.empty(1, dtype=torch.float32, device=dev)      # (a pointer the library never reads)
    y, yp = _i32_rows(targets, dev)
    fn, yn = _i32_lengths(input_length, dev), _i32_lengths(target_length, dev)
    loss = torch.empty((B,), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().vasr_ctc_loss_f32(xp.data_ptr(), fn.data_ptr() if B else None, B, T1, Cn, int(blank),
                                                yp.data_ptr(), y.shape[1], yn.data_ptr() if B else None,
                                                loss.data_ptr() if B else None, _st()))
    return loss


def ctc_align(log_probs, input_length, targets, target_length, blank, want_path=False):
    """Forced (Viterbi) CTC alignment per row (vasr_ctc_align_f32): the best single path of targets[b, :target_length[b]]
    through log_probs[b, :input_length[b]] -> a dict of device tensors: ``score`` [B] f32 (the path's log-probability; -inf
    for a row without a path, a quiet NaN where ``ctc_loss`` gives one), ``start`` / ``end`` [B,W] i32 (token j occupies the
    frames [start, end); -1 behind the row's length and on rows without a path), ``token_logp`` [B,W] f32 (the sum of the
    token's log-probs over its frames; 0 where unfilled) and, with want_path, ``path`` [B,T'] i32 (the state 0 .. 2 L of every
    frame: 2 j + 1 is token j, even states are blanks; -1 from the row's length on).  The arguments, the validation and the
    casts are those of ``ctc_loss``; W <= 4096 (NotImplementedError beyond).  The back-pointer workspace is allocated here.
    Enqueued on the current stream; nothing synchronises."""
    if log_probs.dim() != 3 or not log_probs.dtype.is_floating_point:
        raise ValueError(f"log_probs must be a floating-point [B, T, C] tensor, got {log_probs.dtype} {tuple(log_probs.shape)}")
    if targets.dim() != 2:
        raise ValueError(f"targets must be [B, W], got {tuple(targets.shape)}")
    B, T1, Cn = log_probs.shape
    if targets.shape[0] != B or tuple(torch.as_tensor(input_length).shape) != (B,) or \
            tuple(torch.as_tensor(target_length).shape) != (B,):
        raise ValueError(f"batch sizes differ: log_probs {tuple(log_probs.shape)}, targets {tuple(targets.shape)}, lengths "
                         f"{tuple(torch.as_tensor(input_length).shape)} / {tuple(torch.as_tensor(target_length).shape)}")
    _need_cuda(log_probs)
    dev = log_probs.device
    x = log_probs.detach().to(torch.float32).contiguous()
    xp = x if x.numel() else torch.empty(1, dtype=torch.float32, device=dev)      # (a pointer the library never reads)
    y, yp = _i32_rows(targets, dev)
    W = y.shape[1]
    fn, yn = _i32_lengths(input_length, dev), _i32_lengths(target_length, dev)
    out = {"score": torch.empty((B,), dtype=torch.float32, device=dev),
           "start": torch.empty((B, W), dtype=torch.int32, device=dev), "end": torch.empty((B, W), dtype=torch.int32, device=dev),
           "token_logp": torch.empty((B, W), dtype=torch.float32, device=dev)}
    if want_path:
        out["path"] = torch.empty((B, T1), dtype=torch.int32, device=dev)

    spare = torch.empty(1, dtype=torch.int32, device=dev)    # stands in for an output without storage: never written

    def ptr(name, need=True):
        t = out.get(name)
        if t is None:
            return None
        return t.data_ptr() if t.numel() else (spare.data_ptr() if need else None)

    L = _lib.lib()
    nbytes = L.vasr_ctc_align_workspace_bytes(B, T1, W)       # 0 where the call below refuses its arguments
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check(L.vasr_ctc_align_f32(xp.data_ptr(), fn.data_ptr() if B else None, B, T1, Cn, int(blank), yp.data_ptr(), W,
                                        yn.data_ptr() if B else None, ptr("score") if B else None, ptr("start"), ptr("end"),
                                        ptr("token_logp", need=False), ptr("path", need=False), ws.data_ptr(), nbytes, _st()))
    return out
