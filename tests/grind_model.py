"""The grinding definition in hashlib, and its known
answers.  Everything that grinds -- Channel.grind, fri_grind, fri_grind_batch,
the C++ mirror -- is compared with this model.

    grind(channel, bits, first = 0):
        v = the smallest integer in [first, last] such that
            D = SHA256(ascii(channel.state) || ascii(hex(be64(v))))
            has its `bits` most significant bits zero
        channel.send(be64(v))        # the state becomes D
"""
import functools
import hashlib

S = hashlib.sha256(b"mi355x-fri grind").hexdigest()
assert S == "7318249fdedc258fd28c47e7fce0f9ce31df34032613527ad9bf5b9cd2761396"
LAST = 2 ** 64 - 1


@functools.lru_cache(maxsize=None)
def grind(state: str, bits: int, first: int = 0, last: int = LAST):
    """(nonce, state after the send), or None when [first, last] holds none."""
    head = hashlib.sha256(state.encode())
    for v in range(first, last + 1):
        h = head.copy()
        h.update(b"%016x" % v)
        d = h.digest()
        if int.from_bytes(d[:4], "big") >> (32 - bits) == 0:
            return v, d.hex()
    return None


def zero_bits(state: str) -> int:
    """Leading zero bits of a state (64 hex characters)."""
    return 256 - int(state, 16).bit_length()


# (state, bits, first, nonce, state after the send), computed with hashlib
KATS = [
    ("", 8, 0, 2, "000f6f4ade1994bef54e26f1e2086872e8e49e1fc61d6a67cdf9b53f8cf9fb34"),
    ("", 12, 0, 2, "000f6f4ade1994bef54e26f1e2086872e8e49e1fc61d6a67cdf9b53f8cf9fb34"),
    ("", 16, 0, 40920, "0000c805bc0eda2fe97d2ab2587356fce322d2766c79d3d799c90f0fa60adc85"),
    ("", 20, 0, 2092594, "00000a2b0e21941b33b27f09f24146cb17cd3db08e86a414cda1c14e77cede90"),
    (S, 0, 0, 0, "0db11ab0c8dd44f03ff8f58ad44f8d8c8c8043a782b096e79d6af772971f1e47"),
    (S, 1, 0, 0, "0db11ab0c8dd44f03ff8f58ad44f8d8c8c8043a782b096e79d6af772971f1e47"),
    (S, 8, 0, 347, "00e17f865cd243384b9893a6e46330f522c8d96eb0039385d10704da5e23dafa"),
    (S, 12, 0, 611, "000a324ca7d977d346060340592d4b330dc23252d61307e0d4d7990bf0f15823"),
    (S, 16, 0, 88559, "0000cfda86e16ac0b965bd22917516f29d709adac8fe3e4e0d5984b40e6476d3"),
    (S, 20, 0, 3574556, "00000ef3572afc222cc1081b75e4a3fd84039a15f289e6ed28d6ace58d3471c6"),
    (S, 8, 2 ** 32 - 64, 0x10000003D, "00dbf98ce375a3ac94227f8bbc76c1a8e7292d2be6c366db52be0a2d36c15b08"),
    (S, 12, 2 ** 32 - 64, 0x1000000EF, "0008e11934d97d06e63d20e6cb8537130076934afe69e49aeced6d67e146738f"),
    (S, 8, 2 ** 64 - 4096, 0xFFFFFFFFFFFFF07E, "00d521d9372b4e49628b05bb28deb7f2a57dc8fa29072202057fef043ef33c32"),
]

