"""The shade rules of the results contract (draw order, RC:499-538) are stated once in the kernels' sources: in rt_shade_block.inl, which
rt_shade_phase.inl (the frame, cost and rt_radiance kernels) and rt_radiance_nee_kernel include textually.  A second statement could
drift from the first, so the text itself is checked: no compiler, no assembly."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ray-tracing_amd", "csrc")

# the contract's shade statements, by the marker each carries in the source
MARKERS = ("RC:509 / RC:525", "RC:515", "RC:521", "RC:535-538")


def _sources():
    out = {}
    for pattern in ("*.h", "*.inl", "*.hip"):
        for path in glob.glob(os.path.join(CSRC, pattern)):
            out[os.path.basename(path)] = open(path).read()
    return out


def _includes(text, name):
    return len(re.findall(r'^[ \t]*#[ \t]*include[ \t]+"%s"' % re.escape(name), text, flags=re.M))


def test_each_shade_statement_is_written_once():
    src = _sources()
    assert "rt_shade_block.inl" in src and "rt_shade_phase.inl" in src and "rt_kernels.h" in src
    for marker in MARKERS:
        # not followed by a digit or a range: "RC:515" is not "RC:5150" or "RC:515-518"
        counts = {name: len(re.findall(re.escape(marker) + r"(?![0-9-])", text)) for name, text in src.items()}
        counts = {name: c for name, c in counts.items() if c}
        assert counts == {"rt_shade_block.inl": 1}, (marker, counts)


def test_the_block_and_the_phase_are_included_where_they_should_be():
    src = _sources()
    kernels = src["rt_kernels.h"]
    assert _includes(kernels, "rt_shade_phase.inl") == 3  # trace_body twice, rt_radiance_kernel
    assert _includes(src["rt_shade_phase.inl"], "rt_shade_block.inl") == 1
    assert _includes(kernels, "rt_shade_block.inl") == 1
    for name, text in src.items():
        if name not in ("rt_kernels.h", "rt_shade_phase.inl"):
            assert _includes(text, "rt_shade_block.inl") == 0 and _includes(text, "rt_shade_phase.inl") == 0, name
    # the one direct include of the block is inside rt_radiance_nee_kernel: behind its definition, before the next kernel's
    defs = [(m.start(), m.group(1)) for m in re.finditer(r"^__global__[^\n]*?\b(rt_[a-z0-9_]+_kernel)\(", kernels, flags=re.M)]
    at = re.search(r'^[ \t]*#[ \t]*include[ \t]+"rt_shade_block\.inl"', kernels, flags=re.M).start()
    owner = [name for pos, name in defs if pos < at][-1]
    assert owner == "rt_radiance_nee_kernel", owner
