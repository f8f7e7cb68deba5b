"""Holds tests/_dispatch_arms.py to the host source: every arm of the listed `switch` dispatchers of
zinc_amd/csrc/zip_hip.hip has a census entry and the other way round, and every test the census names exists.  Reads the
project's own host source as text for `case` / `default` labels; no device, no compiled code."""
import os
import re

import pytest

import _dispatch_arms as census

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "zinc_amd", "csrc", "zip_hip.hip")


def function_body(text, name):
    """The text between the braces of the definition of `name`: the first `name(` whose parenthesis closes in front of
    a `{` -- a call's closes in front of `;`, `)` or an operator (comments and string literals must be blanked already)."""
    for m in re.finditer(r"\b%s\s*\(" % re.escape(name), text):
        depth, i = 0, m.end() - 1
        while i < len(text):  # the matching `)`
            depth += {"(": 1, ")": -1}.get(text[i], 0)
            if depth == 0:
                break
            i += 1
        rest = text[i + 1:]
        head = re.match(r"\s*(const\s*)?(noexcept\s*)?(->\s*[\w:<> ]+\s*)?\{", rest)
        if not head:
            continue  # a declaration
        start = i + 1 + head.end()
        depth, j = 1, start
        while depth:
            depth += {"{": 1, "}": -1}.get(text[j], 0)
            j += 1
        return text[start: j - 1]
    raise AssertionError(f"no definition of {name}() in {os.path.relpath(SOURCE, ROOT)}")


def blank_comments_and_strings(src):
    def keep_newlines(m):
        return re.sub(r"[^\n]", " ", m.group(0))

    return re.sub(r"//[^\n]*|/\*.*?\*/|\"(?:\\.|[^\"\\\n])*\"|'(?:\\.|[^'\\\n])+'", keep_newlines, src, flags=re.S)


def switch_labels(body):
    labels = [m.group(1).strip() for m in re.finditer(r"\bcase\s+((?:[^:]|::)+?)\s*:(?!:)", body)]
    labels += ["default"] * len(re.findall(r"\bdefault\s*:", body))
    return labels


@pytest.fixture(scope="module")
def source():
    with open(SOURCE) as fh:
        return blank_comments_and_strings(fh.read())


@pytest.mark.parametrize("name", sorted(census.SWITCHES))
def test_census_lists_exactly_the_arms_of_the_switch(source, name):
    body = function_body(source, name)
    assert len(re.findall(r"\bswitch\s*\(", body)) == 1, f"{name}: the census describes one switch per function"
    labels = switch_labels(body)
    assert len(labels) == len(set(labels)), f"{name}: a label twice"
    listed = set(census.SWITCHES[name])
    for label in sorted(set(labels) - listed):
        pytest.fail(f"{name}: arm `{label}` of the switch has no entry in tests/_dispatch_arms.py")
    for label in sorted(listed - set(labels)):
        pytest.fail(f"{name}: tests/_dispatch_arms.py lists arm `{label}`, the switch has no such label")


def _entries():
    for name, arms in census.SWITCHES.items():
        for label, entry in arms.items():
            yield f"{name} / {label}", entry
    for table in (census.WITH_FL, census.IF_ELSE):
        for name, arms in table.items():
            for label, entry in arms.items():
                yield f"{name} / {label}", entry
    for table in (census.SUMCHECK_PAIRS, census.CLOSED):
        for name, entry in table.items():
            yield name, entry


def test_every_named_test_exists():
    seen = 0
    for where, entry in _entries():
        assert 2 <= len(entry) <= 3 and all(isinstance(x, str) for x in entry[1:]), where
        node = entry[0]
        if node is None:
            assert len(entry) == 3 and entry[2].startswith("unreachable:"), f"{where}: an arm without a test says why"
            continue
        m = re.fullmatch(r"(tests/test_\w+\.py)::(test_\w+)", node)
        assert m, f"{where}: `{node}` is not tests/<file>.py::<test function>"
        path = os.path.join(ROOT, m.group(1))
        assert os.path.isfile(path), f"{where}: {m.group(1)} does not exist"
        with open(path) as fh:
            assert re.search(r"^def %s\(" % m.group(2), fh.read(), flags=re.M), f"{where}: no `def {m.group(2)}` in {m.group(1)}"
        seen += 1
    assert seen > 60


def test_the_parser_sees_a_label_that_is_added():
    """The two ways this census is meant to fail, on a copy of run_combine_extra's switch."""
    src = blank_comments_and_strings(
        "namespace {\nint32_t g(int nt) { /* case 8: */ return f(nt); }\n"
        "int32_t f(uint32_t nt) {\n    switch (nt) {\n        case 1: a(); break;  // case 7:\n"
        "        case Foo::kTwo: b(\"case 5:\"); break;\n        default: c(); break;\n    }\n    return 0;\n}\n}\n")
    assert switch_labels(function_body(src, "f")) == ["1", "Foo::kTwo", "default"]
    assert switch_labels(function_body(src.replace("default:", "case 9: d(); break;\n        default:"), "f")) == ["1", "Foo::kTwo", "9", "default"]
