"""Child interpreter of tests/test_gpu_attention.py for the fp32 route (attention_kernel): knnsvc_wavlm_attention reads
KNNSVC_ATTENTION once per process, so the rows of that route need an interpreter of their own.  Everything else is
tests/attention_child.py restricted to that route.

    python tests/attention_fp32_child.py REPORT.json"""
import os
import sys

os.environ["KNNSVC_ATTENTION"] = "fp32"          # before the library loads (and before attention_child looks)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import attention_child
from tests.gpu_child import run_cases

if __name__ == "__main__":
    sys.exit(run_cases(attention_child.CASES, sys.argv[1]))
