// Multi-member gzip files through the JavaScript host path (streams-api.mjs -> zsnapi.node ->
// zs_pool_inflate_batch_members): decompressBatch*(inputs, "gzip", {outCapacity, members: true}) on members
// that node's own zlib made, one broken stream beside a good one, and the rejection rules.
//   node inflate-members.test.mjs cpu   -- the argument checks only (no GPU needed)
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
  const one = [new Uint8Array(zlib.gzipSync(Buffer.from("x")))];
  const type = (e) => e instanceof TypeError;
  const ok = { outCapacity: 64, members: true };
  for (const format of ["deflate", "deflate-raw", "deflate64-raw"])
    await rejects(api.decompressBatch(one, format, ok), type, format + ": a TypeError");
  await rejects(api.decompressBatch(one, "gzip", { members: true }), type, "without outCapacity: a TypeError");
  await rejects(api.decompressBatchSettled(one, "gzip", { ...ok, dictionary: new Uint8Array(4) }), type, "with a dictionary: a TypeError");
  await rejects(api.decompressBatchDetailed(one, "gzip", { ...ok, restartPoints: "scan" }), type, "with restartPoints: a TypeError");
  await rejects(api.decompressBatchDetailed(one, "gzip", { ...ok, restartPoints: [[[12, 1]]] }), type, "with restart points: a TypeError");
}

const cat = (parts) => new Uint8Array(Buffer.concat(parts.map((p) => Buffer.from(p.buffer, p.byteOffset, p.length))));

async function main() {
  await argumentChecks();
  if (process.argv[2] === "cpu") {
    console.log("ok " + checks);
    return;
  }
  const x = corpus.text(corpus.streamSeed(78), 150000);
  const cuts = [0, 70000, 70005, 150000];
  const parts = [0, 1, 2].map((k) => x.subarray(cuts[k], cuts[k + 1]));
  const gz = (p, level) => new Uint8Array(zlib.gzipSync(Buffer.from(p.buffer, p.byteOffset, p.length), { level }));
  const a = cat(parts.map((p, k) => gz(p, [6, 0, 9][k])));  // three members: the whole text
  const b = cat([gz(x.subarray(0, 100), 6), gz(x.subarray(0, 0), 6), new Uint8Array(13)]);  // an empty member, then padding
  const options = { outCapacity: [150000, 100], members: true };
  const outs = await api.decompressBatch([a, b], "gzip", options);
  expect(same(outs[0], x) && same(outs[1], x.subarray(0, 100)), "two streams, every member");
  const d = await api.decompressBatchDetailed([a, b], "gzip", options);
  expect(d.status[0] === 1 && d.status[1] === 1 && d.consumed[0] === a.length && d.consumed[1] === b.length - 13, "consumed: behind the last trailer");
  // (node's own crc32 where it has one: 20.15 / 22.2 and later)
  expect(typeof zlib.crc32 !== "function" || d.check[0] === zlib.crc32(Buffer.from(x.buffer, x.byteOffset, x.length)) >>> 0,
         "the whole output's crc32");
  // without the option: the first member alone, as ever
  const first = await api.decompressBatch([a], "gzip", { outCapacity: 150000 });
  expect(same(first[0], parts[0]), "the plain call decodes the first member");
  // a flipped CRC byte in the second member fails that stream alone, with the decoder's own message
  const bad = a.slice();
  const m0 = gz(parts[0], 6).length, m1 = gz(parts[1], 0).length;
  bad[m0 + m1 - 8] ^= 1;
  const s = await api.decompressBatchSettled([bad, b], "gzip", options);
  expect(s[0].status === "rejected" && s[0].reason.message === "process error: -3" && s[0].reason.zmsg === "incorrect data check",
         "the failing member's own error");
  expect(s[1].status === "fulfilled" && same(s[1].value, x.subarray(0, 100)), "the neighbour of a broken stream");
  // a total that does not fit
  const t = await api.decompressBatchSettled([a], "gzip", { outCapacity: 149999, members: true });
  expect(t[0].status === "rejected" && t[0].reason.zmsg === "output capacity exceeded", "the capacity outcome");
  console.log("ok " + checks);
}

main().catch((e) => { console.error(e.stack || String(e)); process.exit(1); });
