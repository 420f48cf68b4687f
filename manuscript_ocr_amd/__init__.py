"""manuscript_ocr_amd — MI355X-native hot path of manuscript-ocr (EAST detector + TRBA recogniser)
behind the reference's plugin API: `from manuscript_ocr_amd import Pipeline` replaces
`from manuscript import Pipeline` (/root/reference/src/manuscript/__init__.py:1-4)."""
# The engine keeps several independent launch sequences in flight (detector / recogniser streams of two batches).  The HIP runtime
# multiplexes streams onto a fixed number of hardware queues and a hardware queue runs its kernels in order, so the overlap between
# streams grows with the queue count (DESIGN.md section 7 has the measurements).  The queue count is the runtime's GPU_MAX_HW_QUEUES
# environment variable; the package does not set it: hardware queues are a resource of the machine, shared by every process on the
# card, so the machine's environment decides.
from ._pipeline import Pipeline
from ._search import PageCorpus
from ._spotting import WordIndex
from .detectors import read_image, visualize_page

__all__ = ["Pipeline", "PageCorpus", "WordIndex", "visualize_page", "read_image"]
