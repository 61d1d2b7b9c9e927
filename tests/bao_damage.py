"""Damage cases for the scrub / verify_slice tests: where every node of a bao
combined encoding sits, written bottom-up (pair neighbours level by level,
promote an odd last node) so that it shares nothing with the oracle's
top-down recursion (oracle/pyoracle.py) or with the library's tree
arithmetic, and the closed form of which zfec shards a damaged node spoils."""
from __future__ import annotations

import functools
from typing import NamedTuple


class Node(NamedTuple):
    off: int    # byte offset in the stream
    size: int   # 64 for a parent, the chunk's content bytes for a chunk
    lo: int     # chunk range [lo, hi) below the node
    hi: int
    level: int  # 0 for a chunk, else the pairing round that made the parent

    @property
    def parent(self) -> bool:
        return self.level > 0


def tree_nodes(n: int) -> list[Node]:
    """Every node of the stream over n content bytes, in stream order
    (pre-order: at the same first chunk the wider subtree comes first)."""
    N = max(1, -(-n // 1024))
    spans = [(i, i + 1, 0) for i in range(N)]
    every = list(spans)
    level = 1
    while len(spans) > 1:
        nxt = [(spans[j][0], spans[j + 1][1], level) for j in range(0, len(spans) - 1, 2)]
        every += nxt
        if len(spans) % 2:
            nxt.append(spans[-1])
        spans = nxt
        level += 1
    every.sort(key=lambda s: (s[0], s[0] - s[1]))
    out, off = [], 8
    for lo, hi, lv in every:
        size = 64 if lv else min(1024, n - lo * 1024)
        out.append(Node(off, size, lo, hi, lv))
        off += size
    return out


@functools.lru_cache(maxsize=None)
def chunk_offsets(spc: int) -> tuple[int, ...]:
    """Stream offset of every chunk of a Zfec|Bao stream of eight shards of spc
    chunks each, from tree_nodes."""
    return tuple(nd.off for nd in tree_nodes(8192 * spc) if not nd.parent)


def chunk_off(i: int, N: int) -> int:
    """Stream offset of chunk i of a bao stream of N full chunks (pre-order):
    a walk down from the root, a second derivation that is kept apart from
    chunk_offsets on purpose."""
    off, lo, cnt = 8, 0, N
    while cnt > 1:
        off += 64
        left = 1 << ((cnt - 1).bit_length() - 1)
        if i < lo + left:
            cnt = left
        else:
            off += left * 1024 + 64 * (left - 1)
            lo, cnt = lo + left, cnt - left
    return off


def shards_missing(node: Node, spc: int) -> set[int]:
    """The shards (spc chunks each) whose chunk range misses the node's
    subtree: the ones that stay authentic when only this node is damaged."""
    return {i for i in range(8) if (i + 1) * spc <= node.lo or i * spc >= node.hi}


def every_node_cases(nodes: list[Node]) -> list[tuple[int, int]]:
    """(node number, half) for every parent's left (0) and right (1) half and
    every chunk (half -1): 2 (N - 1) + N cases."""
    cases = []
    for k, nd in enumerate(nodes):
        cases += [(k, 0), (k, 1)] if nd.parent else [(k, -1)]
    return cases


def chosen_node_cases(nodes: list[Node], spc: int) -> list[tuple[int, int]]:
    """The root, the first and last node of every level, every parent that
    straddles a shard boundary, the first and last chunk of every shard; a
    parent's damaged half alternates."""
    pick = {0}
    for lv in {nd.level for nd in nodes}:
        at = [k for k, nd in enumerate(nodes) if nd.level == lv]
        pick |= {at[0], at[-1]}
    for k, nd in enumerate(nodes):
        if nd.parent and any(nd.lo < b * spc < nd.hi for b in range(1, 8)):
            pick.add(k)
        if not nd.parent and (nd.lo % spc == 0 or nd.lo % spc == spc - 1):
            pick.add(k)
    return [(k, j % 2 if nodes[k].parent else -1) for j, k in enumerate(sorted(pick))]


def pick(nodes: list[Node], case: tuple[int, int], rng) -> tuple[int, int]:
    """(stream offset, xor mask) of one bit of the case's node (rng: a
    random.Random, picks byte and bit)."""
    k, half = case
    nd = nodes[k]
    at = rng.randrange(nd.size) if half < 0 else 32 * half + rng.randrange(32)
    return nd.off + at, 1 << rng.randrange(8)


def apply(stream: bytes, flips) -> bytes:
    b = bytearray(stream)
    for pos, mask in flips:
        b[pos] ^= mask
    return bytes(b)


def flip(stream: bytes, nodes: list[Node], case: tuple[int, int], rng) -> bytes:
    """One bit of the case's node flipped."""
    return apply(stream, [pick(nodes, case, rng)])
