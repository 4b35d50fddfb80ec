------------------------------ MODULE mixed_wf ------------------------------
(* Written to show: MIXED FAIRNESS: the waiter is `fair process`, the flipper `fair+ process`, the noise `process`.  The waiter awaits turn = 1 (enabled now and then), the flipper flips the turn (enabled always), the noise flips a bit of its own for ever.  The flipper flips for ever, but the waiter is disabled in every other state: weak fairness obliges it to nothing.  <>(got = 1) is VIOLATED.  The three files of this family differ in the keywords only. *)
EXTENDS Naturals

(* --algorithm mixed_wf
variables turn = 0, got = 0, bit = 0;

fair process Waiter = 0
begin
  W:   await turn = 1;
  Got: got := 1;
end process

fair+ process Flipper = 1
begin
  F: while got = 0 do
       turn := 1 - turn;
     end while;
end process

process Noise = 2
begin
  N: while got = 0 do
       bit := 1 - bit;
     end while;
end process

end algorithm *)

Gets == <>(got = 1)
=============================================================================
