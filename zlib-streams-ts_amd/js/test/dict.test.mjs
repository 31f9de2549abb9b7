// Preset dictionaries through the JavaScript host path (streams-api.mjs ->
// zsnapi.node -> zs_pool_inflate_batch_dict*): decompressBatch*(inputs, format,
// {dictionary}) with one view shared by all inputs or one per input (null = none).
// Inputs are written by node's own zlib against the dictionary.
//   node dict.test.mjs cpu   -- the argument checks only (no GPU needed)
import zlib from "zlib";

import * as corpus from "../../../tests/golden/corpus.mjs";
import * as api from "../streams-api.mjs";

let checks = 0;
const expect = (c, m) => { if (!c) throw new Error("FAIL " + m); checks++; };
const same = (a, b) => a.length === b.length && Buffer.compare(Buffer.from(a.buffer, a.byteOffset, a.length), Buffer.from(b.buffer, b.byteOffset, b.length)) === 0;

async function rejects(p, pred, what) {
  let e = null;
  try { await p; } catch (x) { e = x; }
  expect(e !== null && pred(e), what + (e ? ": " + e.message : ": no error"));
}

async function argumentChecks() {
  const one = [new Uint8Array([3, 0])];
  for (const bad of ["abc", 5, {}, new ArrayBuffer(4)])
    await rejects(api.decompressBatch(one, "deflate-raw", { dictionary: bad }), (e) => e instanceof TypeError,
                  "a non-view dictionary is a TypeError (" + typeof bad + ")");
  await rejects(api.decompressBatch(one, "deflate-raw", { dictionary: ["abc"] }), (e) => e instanceof TypeError,
                "a non-view entry of a per-input dictionary array is a TypeError");
  await rejects(api.decompressBatch(one, "deflate-raw", { dictionary: [null, null] }), (e) => e instanceof TypeError,
                "a per-input dictionary array of the wrong length is a TypeError");
  await rejects(api.decompressBatchDetailed(one, "deflate", { dictionary: "abc" }), (e) => e instanceof TypeError,
                "the detailed entry checks it too");
}

async function main() {
  await argumentChecks();
  if (process.argv[2] === "cpu") {
    console.log("ok " + checks);
    return;
  }
  const dictA = corpus.text(corpus.streamSeed(900), 32768);
  const dictB = corpus.text(corpus.streamSeed(901), 257);
  const recs = [];
  for (let i = 0; i < 64; i++) recs.push(corpus.text(corpus.streamSeed(1000 + i), 100 + 61 * i));
  const level = (i) => [1, 6, 9][i % 3];
  for (const [format, deflate] of [["deflate", zlib.deflateSync], ["deflate-raw", zlib.deflateRawSync]]) {
    // one dictionary shared by all inputs: unbounded and bounded output
    const ins = recs.map((r, i) => new Uint8Array(deflate(r, { dictionary: dictA, level: level(i) })));
    for (const opts of [{ dictionary: dictA }, { dictionary: dictA, outCapacity: 8192 },
                        { dictionary: new DataView(dictA.buffer, dictA.byteOffset, dictA.byteLength) }]) {
      const outs = await api.decompressBatch(ins, format, opts);
      outs.forEach((o, i) => expect(same(o, recs[i]), `${format} shared dictionary, record ${i}`));
    }
    // one per input: A, B or none
    const per = recs.map((r, i) => [dictA, dictB, null][i % 3]);
    const ins2 = recs.map((r, i) => new Uint8Array(per[i] ? deflate(r, { dictionary: per[i], level: level(i) }) : deflate(r, { level: level(i) })));
    const outs2 = await api.decompressBatch(ins2, format, { dictionary: per });
    outs2.forEach((o, i) => expect(same(o, recs[i]), `${format} per-input dictionaries, record ${i}`));
    const det = await api.decompressBatchDetailed(ins2, format, { dictionary: per, outCapacity: 8192 });
    det.outputs.forEach((o, i) => expect(det.status[i] === 1 && same(o, recs[i]) && det.consumed[i] === ins2[i].length,
                                         `${format} detailed, record ${i}`));
    if (format === "deflate")
      recs.forEach((r, i) => expect(det.check[i] === corpus_adler(r), `adler32 of the output only, record ${i}`));
  }
  // the stream layer's error texts: the wrong dictionary, and FDICT without one
  const z = recs.map((r) => new Uint8Array(zlib.deflateSync(r, { dictionary: dictA })));
  await rejects(api.decompressBatch(z, "deflate", { dictionary: dictB }), (e) => e.message === "process error: -3",
                "wrong dictionary");
  await rejects(api.decompressBatch(z, "deflate", { dictionary: z.map(() => null) }), (e) => e.message === "process error: 2",
                "FDICT without a dictionary");
  await rejects(api.decompressBatch(z, "deflate"), (e) => e.message === "process error: 2", "FDICT, no dictionary option");
  const settled = await api.decompressBatchSettled(z, "deflate", { dictionary: z.map((_, i) => (i % 2 ? dictA : dictB)) });
  settled.forEach((s, i) => expect(i % 2 ? s.status === "fulfilled" && same(s.value, recs[i])
                                         : s.status === "rejected" && s.reason.message === "process error: -3" && s.reason.zmsg === "",
                                   `settled ${i}`));
  await rejects(api.decompressBatch(z, "gzip", { dictionary: dictA }), (e) => e.code === "-2", "gzip takes no dictionary");
  console.log("ok " + checks);
}

function corpus_adler(b) {
  let a = 1, s = 0;
  for (let i = 0; i < b.length; i++) {
    a = (a + b[i]) % 65521;
    s = (s + a) % 65521;
  }
  return ((s << 16) | a) >>> 0;
}

main().catch((e) => { console.error(e); process.exit(1); });
