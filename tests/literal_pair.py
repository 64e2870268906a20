"""Which pair of libraries this process tests, and the tally the gate suites keep of what they compared.

The product pair is syzygy_amd/csrc/libszg_hip.so against oracle/libszg_oracle.so. The literal pair is libszg_hip_literal.so
(the same kernels compiled with -DSZG_LITERAL: no a * b + c is fused) against libszg_oracle_literal.so, and with them the
*_literal.so harnesses of tests/Makefile. A process tests the literal pair when BOTH variables say so:

    SZG_ORACLE_LITERAL=1                          (oracle/binding.py)
    SZG_HIP_LIBRARY=<...>/libszg_hip_literal.so   (syzygy_amd/_lib.py)

With neither set it tests the product pair. Anything between the two - one variable without the other, SZG_ORACLE_LITERAL
with another value than "1", the literal oracle against another library - is refused: a half-literal run compares two
different programs and its failures, or its passes, mean nothing. Only tests/test_gpu_literal_gates.py sets the variables,
for its child processes (tests/gpu_literal_gates_child.py)."""
import contextlib
import os

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LITERAL_HIP = "libszg_hip_literal.so"
LITERAL_ORACLE = "libszg_oracle_literal.so"


def pair(environ=None):
    """"product" or "literal", from the environment; ValueError for an environment that names half a pair."""
    env = os.environ if environ is None else environ
    oracle = env.get("SZG_ORACLE_LITERAL")
    library = env.get("SZG_HIP_LIBRARY")
    literal_oracle = oracle == "1"
    literal_library = bool(library) and os.path.basename(library) == LITERAL_HIP
    if oracle not in (None, "", "1"):
        raise ValueError(f"SZG_ORACLE_LITERAL={oracle!r}: oracle/binding.py switches to the literal oracle for '1' alone; "
                         "set it to 1 or unset it")
    if literal_oracle and literal_library:
        return "literal"
    if literal_oracle:
        raise ValueError(f"SZG_ORACLE_LITERAL=1 asks for the literal oracle, but SZG_HIP_LIBRARY={library!r} does not name "
                         f"{LITERAL_HIP}: set both variables for the literal pair, or neither for the product pair")
    if literal_library:
        raise ValueError(f"SZG_HIP_LIBRARY={library!r} names the literal kernels, but SZG_ORACLE_LITERAL is not 1: set both "
                         "variables for the literal pair, or neither for the product pair")
    return "product"


def literal_environment(environ=None):
    """A copy of the environment with the two variables of the literal pair set."""
    env = dict(os.environ if environ is None else environ)
    env["SZG_ORACLE_LITERAL"] = "1"
    env["SZG_HIP_LIBRARY"] = os.path.join(ROOT, "syzygy_amd", "csrc", LITERAL_HIP)
    return env


# ---------------------------------------------------------------------------------------------------------------------
# The tally. Every bit-for-bit comparison of the gate suites reports how many values it is about to hold to the oracle
# (compared(n)), BEFORE it asserts. Nobody listens unless a tally is open: the suites' own tests run as they always did.
# tests/gpu_literal_gates_child.py opens one per group and so learns how much a group compared, also when it failed.
# ---------------------------------------------------------------------------------------------------------------------
class Tally:
    def __init__(self):
        self.compared = 0


_OPEN = []


def compared(values):
    """`values` values (floats of a debug image or a march result, channels of a UNORM16 colour) are compared bit for bit."""
    for t in _OPEN:
        t.compared += int(values)


@contextlib.contextmanager
def tally():
    t = Tally()
    _OPEN.append(t)
    try:
        yield t
    finally:
        _OPEN.remove(t)
