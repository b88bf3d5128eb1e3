# -*- coding: utf-8 -*-
"""ssqueezepy_amd -- MI355X-native synchrosqueezed CWT / STFT engine.

Drop-in for the transform path of ssqueezepy (`cwt`, `stft`, `ssq_cwt`, `ssq_stft`,
`ssqueeze`, `phase_cwt`, `phase_stft`, their inverses `icwt`, `issq_cwt`, `istft`,
`issq_stft`, `extract_ridges`, `trigdiff`, `phase_ssqueeze`, `Wavelet` and the scale-design
utilities): same Python API, computed by hand-written HIP kernels (gfx950) behind a
C ABI (include/ssq_hip.h, libssq_hip.so). The design step (scales, filter bank,
frequency grid, windows) is host NumPy and value-exact with the reference; all
O(na * N) work is on the GPU and there is no CPU fallback.
"""
__version__ = '0.1.0'

from .configs import EPS32, EPS64, USE_GPU, IS_PARALLEL
from .padding import p2up, padsignal
from .wavelets import Wavelet, center_frequency
from .scales import (process_scales, make_scales, cwt_scalebounds, infer_scaletype,
                     logscale_transition_idx, adm_ssq, adm_cwt)


def __getattr__(name):
    # the compute layer needs torch + the HIP library; import it lazily so that the
    # host-side design modules stay importable on a machine without a GPU
    _lazy = {
        'cwt': '_cwt', 'cwt_higher_order': '_cwt', 'ssq_cwt': '_ssq_cwt', 'phase_cwt': '_ssq_cwt',
        'stft': '_stft', 'get_window': '_stft', 'ssq_stft': '_ssq_stft',
        'phase_stft': '_ssq_stft', 'ssq_stft2': '_ssq_stft2', 'ssq_cwt2': '_ssq_cwt2', 'ssqueeze': 'ssqueezing',
        'conceft_stft': '_conceft', 'hermite_windows': '_conceft', 'conceft_gpu': 'algos',
        'conceft_cwt': '_conceft_cwt', 'morse_wavelets': 'wavelets', 'conceft_cwt_gpu': 'algos',
        'tssq_stft': '_tssq_stft', 'time_reassign_gpu': 'algos',
        'msst_stft': '_msst_stft', 'multi_squeeze_gpu': 'algos',
        'msst_cwt': '_msst_cwt', 'multi_squeeze_cwt_gpu': 'algos', 'row_frequencies': 'wavelets',
        'reassign_stft': '_reassign_stft', 'reassign2d_gpu': 'algos',
        'reassign_cwt': '_reassign_cwt', 'reassign_cwt_gpu': 'algos', 'wavelet_time_std': 'wavelets',
        'tssq_cwt': '_tssq_cwt', 'time_reassign_cwt_gpu': 'algos', 'cwt_rotation_tables': 'algos',
        'ssqueeze_fast': 'algos', 'indexed_sum_onfly': 'algos', 'buffer': 'algos',
        'replace_under_abs': 'algos', 'phase_cwt_gpu': 'algos',
        'phase_stft_gpu': 'algos', 'phase_stft2_gpu': 'algos', 'phase_cwt2_gpu': 'algos',
        'icwt': '_inverse', 'issq_cwt': '_inverse', 'istft': '_inverse',
        'issq_stft': '_inverse', 'extract_ridges': 'ridge_extraction',
        'freq_to_scale': 'experimental', 'scale_to_freq': 'experimental', 'trigdiff': 'common',
        'phase_ssqueeze': 'experimental', 'phase_transform': 'experimental',
    }
    if name in _lazy:
        import importlib
        mod = importlib.import_module('.' + _lazy[name], __name__)
        obj = getattr(mod, name)
        globals()[name] = obj          # later look-ups find it directly (the import costs ~5 us per call)
        return obj
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
