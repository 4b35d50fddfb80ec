------------------------------ MODULE toggle_fair ------------------------------
(* Written to show: A TOGGLER / WAITER PAIR, the waiter declared `fair process`.  The waiter awaits turn = 1 while a fair toggler flips the turn until the waiter got through.  The waiter is enabled in every other state of the toggler's cycle: weak fairness obliges it to nothing, strong fairness makes it move.  Termination is VIOLATED.  The twin file differs in the waiter's keyword only. *)
EXTENDS Naturals

(* --algorithm toggle_fair
variables turn = 0, got = 0;

fair process Waiter = 0
begin
  W:   await turn = 1;
  Got: got := 1;
end process

fair process Toggler = 1
begin
  F: while got = 0 do
       turn := 1 - turn;
     end while;
end process

end algorithm *)

=============================================================================
