"""proto_clip_amd — MI355X (gfx950) implementation of Proto-CLIP's data-parallel hot path: CLIP encoder
forwards that fill the memory banks, the per-class prototype reduction, query adapters, and the
dual-bank distance-softmax classification, behind the reference's Python surface (main.py / model.py /
utils.py / clip).  Arithmetic runs in libpclip.so (hand-written HIP, C ABI in include/pclip.h);
importing this package needs no GPU, calling into it does."""
__version__ = "0.1.0"

from . import _lib  # noqa: F401  (ctypes binding; the shared library is loaded on first use)
from ._lib import PclipError  # noqa: F401
from . import tip_adapter  # noqa: F401,E402  (the Tip-Adapter / Tip-Adapter-F baselines: tip_logits, tip_classify, search_hp, TipAdapterF, run_tip_adapter[_F])
from . import vpt  # noqa: F401,E402  (visual prompt tuning through the frozen vision tower: VisualPromptLearner, VPT, run_vpt)
from . import maple  # noqa: F401,E402  (multi-modal prompt learning, deep text prompts coupled to VPT: MultiModalPromptLearner, MaPLe, run_maple)
from .maple import MaPLe, MultiModalPromptLearner, run_maple  # noqa: F401,E402
from . import cocoop  # noqa: F401,E402  (the image-conditioned context: ConditionalPromptLearner, CoCoOp, run_cocoop)
from .cocoop import CoCoOp, ConditionalPromptLearner, run_cocoop  # noqa: F401,E402
from . import prograd  # noqa: F401,E402  (prompt-aligned gradient: CoOp with a KL to the zero-shot classifier and the gradient projection: ProGrad, run_prograd)
from .prograd import ProGrad, run_prograd  # noqa: F401,E402
from . import promptsrc  # noqa: F401,E402  (self-regulated prompts: independent deep prompts, feature and logit regularisers, Gaussian aggregation: PromptSRC, run_promptsrc)
from .promptsrc import IndependentPromptLearner, PromptSRC, run_promptsrc  # noqa: F401,E402
