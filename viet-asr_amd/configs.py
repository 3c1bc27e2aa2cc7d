"""Model definitions for the three QuartzNet variants the reference ships, plus a loader
for reference-format YAML files.

The reference reads ``configs/*.yaml`` with ruamel and splats the sections into the module
constructors (infer.py:85-111).  ``load_model_definition`` accepts exactly those files (and the
legacy ``AudioPreprocessing`` section name that configs/quartznet15x5.yaml:16-26 still uses);
``builtin(name)`` rebuilds the same dictionaries from a compact table so that the GPU box --
where /root/reference does not exist -- needs no data files.
"""
import copy

import yaml

# label sets (configs/quartznet12x1_vi.yaml:166-, quartznet15x5.yaml:201-, quartznet12x1.yaml)
LABELS_VI = list(" abcdeghiklmnopqrstuvxyàáâãèéêìíòóôõùúýăđĩũơưạảấầẩẫậắằẳẵặẹẻẽếềểễệỉịọỏốồổỗộớờởỡợụủứừửữựỳỵỷỹ")
LABELS_EN = list(" abcdefghijklmnopqrstuvwxyz'")
LABELS_VI_DIGITS = list(" 0123456789aáàảãạăắằẳẵặâấầẩẫậbcdđeéèẻẽẹfghiíìỉĩịjklmnoóòỏõọôốồổỗộơớờởỡợpqrstuúùủũụưứừửữựvxyýỳỷỹỵz")

_PRE = dict(sample_rate=16000, window_size=0.02, window_stride=0.01, window="hann", normalize="per_feature",
            n_fft=512, features=64, dither=0.00001, pad_to=16, stft_conv=False)


def _blk(filters, repeat, kernel, stride=1, dilation=1, residual=True, separable=True, residual_dense=False):
    d = dict(filters=filters, repeat=repeat, kernel=[kernel], stride=[stride], dilation=[dilation],
             dropout=0.0, residual=residual)
    if separable:
        d["separable"] = True
    if residual_dense:
        d["residual_dense"] = True
    return d


def _jasper10x5dr():
    """Jasper 10x5 with dense residuals (Jasper paper, table 1 and section 2.2): a K 11 stride-2 prologue, B1-B5 x2 of five
    non-separable sub-blocks each (256 / K 11, 384 / 13, 512 / 17, 640 / 21, 768 / 25), every one residual and dense, then a
    K 29 dilation-2 and a K 1 epilogue block, as NeMo's jasper10x5dr.yaml of this generation spells it."""
    blocks = [_blk(256, 1, 11, stride=2, residual=False, separable=False)]
    for ch, k in ((256, 11), (384, 13), (512, 17), (640, 21), (768, 25)):
        blocks += [_blk(ch, 5, k, separable=False, residual_dense=True) for _ in range(2)]
    blocks += [_blk(896, 1, 29, dilation=2, residual=False, separable=False),
               _blk(1024, 1, 1, residual=False, separable=False)]
    return blocks


def _quartznet(repeat, with_dilated_tail):
    """B1..B5 x3 QuartzNet body (QuartzNet paper table 1) as the reference YAMLs spell it."""
    blocks = [_blk(256, 1, 33, stride=2, residual=False)]
    for ch, k in ((256, 33), (256, 39), (512, 51), (512, 63), (512, 75)):
        if (ch, k) == (512, 75) and not with_dilated_tail:
            blocks += [_blk(ch, repeat, k)]            # 12x1: a single K=75 block
        else:
            blocks += [_blk(ch, repeat, k) for _ in range(3)]
    if with_dilated_tail:
        blocks.append(_blk(512, 1, 87, dilation=2, residual=False))
    blocks.append(_blk(1024, 1, 1, residual=False, separable=False))
    return blocks


def builtin(name):
    """Model definition dict equal to yaml-loading the reference config of that name -- with one deliberate exception:
    configs/quartznet15x5.yaml:26 says ``stft_conv: true`` (the third-party torch_stft package, absent here and on the
    reference side of the golden generator); the builtin 15x5 keeps ``stft_conv=False`` like the two Vietnamese configs,
    which is how tests/golden/make_golden.py runs the reference.  Loading the real YAML selects the conv-STFT's
    periodic window (frontend_tables.frontend_description)."""
    # trim: the YAML's AudioToTextDataLayer.trim_silence (quartznet15x5.yaml:6 true; quartznet12x1*.yaml false) -- what
    # VietASR's trim_silence="config" follows
    trim = False
    if name in ("quartznet12x1_vi", "quartznet12x1_vi.yaml"):
        body, labels = _quartznet(1, False), LABELS_VI
    elif name in ("quartznet12x1", "quartznet12x1.yaml"):
        body, labels = _quartznet(1, False), LABELS_VI_DIGITS
    elif name in ("quartznet15x5", "quartznet15x5.yaml"):
        body, labels, trim = _quartznet(5, True), LABELS_EN, True
    elif name in ("jasper10x5dr", "jasper10x5dr.yaml"):
        body, labels = _jasper10x5dr(), LABELS_EN
    else:
        raise ValueError(f"unknown builtin model {name!r}")
    d = {
        "model": name.replace(".yaml", ""),
        "AudioToTextDataLayer": {"max_duration": 16.7, "trim_silence": trim},
        "AudioToMelSpectrogramPreprocessor": dict(_PRE),
        "JasperEncoder": {"activation": "relu", "conv_mask": True, "jasper": body},
        "labels": list(labels),
    }
    if d["model"] in _SPEC_AUGMENT:
        d["SpectrogramAugmentation"] = dict(_SPEC_AUGMENT[d["model"]])
    return d


# the SpectrogramAugmentation section of every shipped YAML (quartznet15x5.yaml:28-31, quartznet12x1.yaml:25-28,
# quartznet12x1_vi.yaml:20-23): constructor arguments of asr.SpectrogramAugmentation
_SPEC_AUGMENT = {name: {"rect_masks": 5, "rect_time": 120, "rect_freq": 50}
                 for name in ("quartznet15x5", "quartznet12x1", "quartznet12x1_vi")}


def spectrogram_augmentation(name):
    """The ``SpectrogramAugmentation`` section of the shipped config of that name (a new dict), or None where the reference
    ships none (jasper10x5dr)."""
    model = builtin(name)["model"]          # (unknown names: ValueError)
    return dict(_SPEC_AUGMENT[model]) if model in _SPEC_AUGMENT else None


def jasper_definition(jasper, labels=None):
    """Model definition around a block list (JasperEncoder.jasper): the builtin front end, English labels by default."""
    return {
        "model": "custom",
        "AudioToMelSpectrogramPreprocessor": dict(_PRE),
        "JasperEncoder": {"activation": "relu", "conv_mask": True, "jasper": copy.deepcopy(list(jasper))},
        "labels": list(labels or LABELS_EN),
    }


def normalize_definition(d):
    """Accept both section spellings; drop keys the mel preprocessor never had (feat_type)."""
    d = copy.deepcopy(d)
    if "AudioToMelSpectrogramPreprocessor" not in d and "AudioPreprocessing" in d:
        pre = dict(d.pop("AudioPreprocessing"))
        pre.pop("feat_type", None)
        pre.setdefault("sample_rate", d.get("sample_rate", 16000))
        d["AudioToMelSpectrogramPreprocessor"] = pre
    return d


def load_model_definition(path):
    with open(path, encoding="utf-8") as f:
        return normalize_definition(yaml.safe_load(f))
